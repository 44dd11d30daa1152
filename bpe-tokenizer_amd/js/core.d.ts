// core.d.ts — type surface of the drop-in core.js; identical to beenotung/bpe-tokenizer v2.2.0
// core.ts (types core.ts:1-33, exports core.ts:36-75, class core.ts:77-495, compactMerge 500-503).
export type Token = {
  chars: string
  /** @description the weight after merge */
  weight: number
  /** @description the weight before merge */
  original_weight: number
  code: string
  /** @description including zero-weight tokens in token_table */
  index: number
}
export type MergeToken = [a: Token, b: Token, c: Token]
export type CompactMerge = [a_code: string, b_code: string, c_weight: number]
type MergeCode = [from_code: string, to_code: string]
export type BPETokenizerJSON = {
  version: 2
  char_count: number
  token_table: [chars: string, weight: number, original_weight: number][]
  merge_codes: [a_code: string, b_code: string, c_code: string][]
}
export declare let FS: string
export declare let EOF: string
export declare let LF: string
export declare let CR: string
export type Markers = {
  begin_marker: string
  end_marker: string
}
export declare function fileContentToCorpus(content: string | Buffer): string
export type CorpusHelperName = 'linesToCorpus' | 'linesTrimmedToCorpus' | 'fileContentToCorpus'
/** two planes of vector indices and one pair offset per text, plus the total */
export type SkipGramPairs = { targets: Int32Array; contexts: Int32Array; offsets: Float64Array }
export declare function linesToCorpus(text: string): string[]
export declare function linesTrimmedToCorpus(text: string): string[]
export declare class BPETokenizer {
  char_to_token: Record<string, Token>
  code_to_token: Record<string, Token>
  token_table: Token[]
  merge_tokens: MergeToken[]
  merge_codes: MergeCode[]
  to_vector_index: number[] | null
  from_vector_index: number[] | null
  /** materialised from HBM on read; assigning replaces the device corpus (`= []` clears it) */
  corpus_in_code: string[]
  toJSON(): BPETokenizerJSON
  fromJSON(json: BPETokenizerJSON): void
  protected invalidateVectorIndex(): void
  addToCorpus(content: string): void
  restoreToCorpus(content: string): void
  compactVectorIndex(): void
  findNextMerge(options?: { min_weight?: number; max_length?: number }): MergeToken | null
  applyMerge(merge: MergeToken): void
  mergeUntil(options?: { min_weight?: number; max_length?: number; max_iterations?: number }): void
  encodeToCode(content: string): string
  encodeToTokens(content: string): Token[]
  encodeToVector(content: string): number[]
  decodeTokens(tokens: Token[]): string
  decodeVector(vector: number[]): string
  /**
   * decodeVector for many vectors at once on the GPU: equals `vectors.map(v => this.decodeVector(v))`,
   * the `unknown vector index: V` error included.  Needs a HIP device.
   */
  decodeVectorBatch(vectors: number[][]): string[]
  /**
   * decodeVectorBatch as UTF-8 bytes, encoded on the GPU as `Buffer.from(text)` encodes them (a lone
   * surrogate becomes EF BF BD): equals `this.decodeVectorBatch(vectors).map(s => Buffer.from(s))`.
   * The Buffers are slices of one allocation.  Without a HIP device the strings are encoded on the host.
   */
  decodeVectorBatchUtf8(vectors: number[][]): Buffer[]
  /**
   * encodeToVector for many texts at once on the GPU: equals `texts.map(t => this.encodeToVector(t))`,
   * the `unknown token, char: ...` and `unknown token index: N` errors included.  Without a HIP
   * device (or with BPE_ENCODE_DEVICE=0) that map runs in JS.
   */
  encodeToVectorBatch(texts: string[]): number[][]
  /**
   * addToCorpus for many contents at once on the GPU: leaves the tables, toJSON() and the corpus as
   * `for (let c of contents) this.addToCorpus(c)` would.  Needs a HIP device.
   */
  addToCorpusBatch(contents: string[]): void
  /**
   * restoreToCorpus for many contents at once on the GPU: leaves the corpus as
   * `for (let c of contents) this.restoreToCorpus(c)` would, except that the batch is atomic (an
   * unknown char throws `unknown token, char: ...` and adds no content).  Without a HIP device (or
   * with BPE_ENCODE_DEVICE=0) that loop runs in JS.
   */
  restoreToCorpusBatch(contents: string[]): void
  /**
   * the three batch methods for UTF-8 bytes (files, datasets), decoded on the GPU exactly as
   * `buffer.toString()` decodes them: ill-formed bytes become U+FFFD, a char like any other.  Each
   * leaves the tokenizer as the method above does on `buffers.map(b => b.toString())`: weights,
   * char_to_token, token_table order and error strings.  addToCorpusBatchUtf8 needs a HIP device;
   * the other two run that map in JS without one.
   */
  addToCorpusBatchUtf8(buffers: Array<Buffer | Uint8Array>): void
  restoreToCorpusBatchUtf8(buffers: Array<Buffer | Uint8Array>): void
  encodeToVectorBatchUtf8(buffers: Array<Buffer | Uint8Array>): number[][]
  /**
   * The corpus helpers on the GPU: every text (file) is split into samples by `helper` (default
   * 'linesToCorpus') on the device and ingested or restored there; the tokenizer is left exactly as
   * `texts.flatMap(helper).forEach(s => t.addToCorpus(s))` (or restoreToCorpus) leaves it.  They need
   * a HIP device; any other helper name throws.
   */
  addLinesToCorpusBatch(texts: string[], helper?: CorpusHelperName): void
  addLinesToCorpusBatchUtf8(buffers: Array<Buffer | Uint8Array>, helper?: CorpusHelperName): void
  restoreLinesToCorpusBatch(texts: string[], helper?: CorpusHelperName): void
  restoreLinesToCorpusBatchUtf8(buffers: Array<Buffer | Uint8Array>, helper?: CorpusHelperName): void
  /**
   * the trained corpus as vectors on the GPU: `encodeToVector` of every training sample (of the samples
   * `indices`, in that order, when given) without encoding the raw text again; throws
   * `unknown token index: N`.  Without the addon (or with BPE_ENCODE_DEVICE=0) the map runs in JS.
   */
  corpusToVectorBatch(indices?: number[]): Int32Array[]
  /**
   * the trained corpus back as text on the GPU: the contents of the samples (`indices` when given).
   * Without the addon (or with BPE_ENCODE_DEVICE=0) the chars are joined in JS.
   */
  corpusToTextBatch(indices?: number[]): string[]
  /**
   * corpusToTextBatch as UTF-8 bytes, encoded on the GPU: equals
   * `this.corpusToTextBatch(indices).map(s => Buffer.from(s))`.  The Buffers are slices of one
   * allocation.  Without the addon (or with BPE_ENCODE_DEVICE=0) the strings are encoded on the host.
   */
  corpusToTextBatchUtf8(indices?: number[]): Buffer[]
  /**
   * skip-gram training pairs on the GPU: the (target, context) pairs the loop of example/skip-gram.ts
   * makes of `encodeToVector(text)` over `window` (default 2, at most 64) values on each side, for many
   * texts, UTF-8 buffers or corpus samples at once; text k owns the pairs offsets[k] .. offsets[k + 1].
   * The errors are those of encodeToVectorBatch and corpusToVectorBatch.  When the device cannot take a
   * call, their vectors are expanded in JS.
   */
  skipGramBatch(texts: string[], window?: number): SkipGramPairs
  skipGramBatchUtf8(buffers: Array<Buffer | Uint8Array>, window?: number): SkipGramPairs
  corpusToSkipGramBatch(indices?: number[] | null, window?: number): SkipGramPairs
  restoreMerge(compactMerge: CompactMerge): void
}
export declare function compactMerge(merge: MergeToken): CompactMerge
export {}
