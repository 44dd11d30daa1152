'use strict'
/**
 * native.js — internal: the N-API addon (addon/bpe_napi.node) and the option conventions shared
 * by the two drop-ins, core.js (BPETokenizer) and db.js (BPETokenizerDB).
 */
const path = require('path')

let native = null
function loadNative() {
  if (!native) native = require(path.join(__dirname, '..', 'addon', 'bpe_napi.node'))
  return native
}

// the decoder's addon (addon/bpe_decode_napi.node: createDecoder ... decodeBatch)
let nativeDecode = null
function loadNativeDecode() {
  if (!nativeDecode) nativeDecode = require(path.join(__dirname, '..', 'addon', 'bpe_decode_napi.node'))
  return nativeDecode
}

// the text ingest's addon (addon/bpe_ingest_napi.node: setChars, addTextBatch on an engine handle)
let nativeIngest = null
function loadNativeIngest() {
  if (!nativeIngest) nativeIngest = require(path.join(__dirname, '..', 'addon', 'bpe_ingest_napi.node'))
  return nativeIngest
}

// the restore's addon (addon/bpe_restore_napi.node: addSampleBatch, restoreTextBatch on an engine handle)
let nativeRestore = null
function loadNativeRestore() {
  if (!nativeRestore) nativeRestore = require(path.join(__dirname, '..', 'addon', 'bpe_restore_napi.node'))
  return nativeRestore
}

// the UTF-8 addon (addon/bpe_utf8_napi.node: addUtf8Batch, restoreUtf8Batch on an engine handle,
// encodeUtf8Batch on a text encoder handle)
let nativeUtf8 = null
function loadNativeUtf8() {
  if (!nativeUtf8) nativeUtf8 = require(path.join(__dirname, '..', 'addon', 'bpe_utf8_napi.node'))
  return nativeUtf8
}

// the addon of the corpus helpers on the device (addon/bpe_lines_napi.node: addLinesBatch,
// addLinesUtf8Batch, restoreLinesBatch, restoreLinesUtf8Batch on an engine handle)
let nativeLines = null
function loadNativeLines() {
  if (!nativeLines) nativeLines = require(path.join(__dirname, '..', 'addon', 'bpe_lines_napi.node'))
  return nativeLines
}

// the corpus helpers by name -> BPE_LINES_TRIM, BPE_LINES_KEEP, BPE_LINES_FILE (include/bpe.h)
const LINES_HELPERS = { linesToCorpus: 0, linesTrimmedToCorpus: 1, fileContentToCorpus: 2 }
function linesMode(helper) {
  let name = helper === undefined ? 'linesToCorpus' : helper
  if (typeof name !== 'string' || !Object.prototype.hasOwnProperty.call(LINES_HELPERS, name))
    throw new Error(
      'unknown corpus helper: ' + String(helper) + ' (linesToCorpus, linesTrimmedToCorpus or fileContentToCorpus)',
    )
  return LINES_HELPERS[name]
}

// the addon of the ways out as UTF-8 (addon/bpe_utf8_out_napi.node: decodeUtf8Batch on a decoder
// handle, exportUtf8 on an engine handle and a decoder handle)
let nativeUtf8Out = null
function loadNativeUtf8Out() {
  if (!nativeUtf8Out) nativeUtf8Out = require(path.join(__dirname, '..', 'addon', 'bpe_utf8_out_napi.node'))
  return nativeUtf8Out
}

// the text encoder's addon (addon/bpe_text_napi.node: createTextEncoder ... encodeTextBatch)
// the export's addon (addon/bpe_export_napi.node: exportSamples, exportText on an engine handle)
let nativeExport = null
let nativeExportMissing = false
function loadNativeExport() {
  if (!nativeExport) nativeExport = require(path.join(__dirname, '..', 'addon', 'bpe_export_napi.node'))
  return nativeExport
}

// the skip-gram addon (addon/bpe_skipgram_napi.node: skipGramTextBatch and skipGramUtf8Batch on a
// text encoder handle, exportSkipGram on an engine handle)
let nativeSkipGram = null
function loadNativeSkipGram() {
  if (!nativeSkipGram) nativeSkipGram = require(path.join(__dirname, '..', 'addon', 'bpe_skipgram_napi.node'))
  return nativeSkipGram
}

let nativeText = null
function loadNativeText() {
  if (!nativeText) nativeText = require(path.join(__dirname, '..', 'addon', 'bpe_text_napi.node'))
  return nativeText
}

/**
 * encodeToCode (core.ts:392-409) runs on the GPU (bpe_encode_batch: the merge-rank encoder for
 * texts up to ENCODE_LDS_TOKENS tokens, apply-only replay passes above) when a per-call cost model
 * fitted to the measured crossover (profiles/r04_encode_crossover.json, MI355X + Node on the box's
 * host) says it beats the reference's own replay (one split/join per merge, kept below):
 *   JS replay     ~ 0.11 us per merge + chars x (0.03 + 0.00005 x merges) us
 *   device (LDS)  ~ 30 us per call + 1.6 us per greedy step (at most min(merges, 0.4 x chars))
 *                   + 0.05 us per char (id and code conversions, copies)
 *   device (long) ~ 10 us per merge (one replay pass each) + 0.05 us per char
 * In practice: long merge lists with short texts, and long texts.  BPE_ENCODE_DEVICE=0 keeps every
 * call on the JS replay, =1 sends every call with a merge to the device and lets its errors through
 * (tests).  By default a call the device cannot take falls back to the JS replay
 * (encodeIdsMaybeOnDevice): no addon or no HIP device (remembered for the owner's lifetime), or a
 * merge list with a token id the device encoder does not hold (>= BPE_MAX_VOCAB: remembered while
 * the owner keeps that list), so the drop-in encodes wherever the reference does.
 */
const ENCODE_LDS_TOKENS = 16384
const ENCODE_DEVICE = process.env.BPE_ENCODE_DEVICE

function encodeOnDevice(n_chars, n_merges) {
  if (n_chars < 2 || n_merges < 1 || ENCODE_DEVICE === '0') return false
  if (ENCODE_DEVICE === '1') return true
  const js = 0.11 * n_merges + n_chars * (0.03 + 0.00005 * n_merges)
  const dev =
    n_chars <= ENCODE_LDS_TOKENS
      ? 30 + 1.6 * Math.min(n_merges, 0.4 * n_chars) + 0.05 * n_chars
      : 10 * n_merges + 0.05 * n_chars
  return dev < js
}

/**
 * The owner's device encoder (bpe_encoder_*), holding the merge list `list` as a rank table; the
 * merges appended to the list since the last call are appended to it (applyMerge, restoreMerge,
 * mergeUntil), and a replaced or shortened list (fromJSON) rebuilds it.  tripleOf(entry) -> the
 * entry's (a, b, c) token indices.  The owner keeps the handle in non-enumerable fields.
 */
function syncEncoder(owner, list, tripleOf) {
  let n = loadNative()
  if (!owner._encoder) {
    for (let k of ['_encoder', '_enc_list', '_enc_n', '_enc_last'])
      if (!Object.prototype.hasOwnProperty.call(owner, k))
        Object.defineProperty(owner, k, { value: null, writable: true, enumerable: false })
    owner._encoder = n.createEncoder(0)
    owner._enc_list = null
  }
  let have = owner._enc_n || 0
  if (owner._enc_list !== list || have > list.length || (have && list[have - 1] !== owner._enc_last)) {
    n.encoderClear(owner._encoder)
    owner._enc_list = list
    have = 0
  }
  if (have < list.length) {
    let k = list.length - have
    let abc = new Int32Array(3 * k)
    for (let i = 0; i < k; i++) {
      let t = tripleOf(list[have + i])
      abc[3 * i] = t[0]
      abc[3 * i + 1] = t[1]
      abc[3 * i + 2] = t[2]
    }
    n.encoderAddMerges(owner._encoder, abc)
  }
  owner._enc_n = list.length
  owner._enc_last = list.length ? list[list.length - 1] : null
  return owner._encoder
}

/** one text's token ids through the owner's merges on the device -> Int32Array of ids */
function encodeIdsOnDevice(owner, list, tripleOf, ids) {
  let enc = syncEncoder(owner, list, tripleOf)
  let res = loadNative().encodeBatch(enc, Int32Array.from(ids), Float64Array.of(0, ids.length))
  return res[0]
}

/**
 * encodeIdsMaybeOnDevice when the cost model sends the call to the device and the device can take it,
 * else null (the caller then runs the reference's replay).  Only what the device cannot do is
 * remembered on the owner (non-enumerable `_enc_failed`): `true` when the encoder itself cannot be
 * made (no addon, no HIP device), the list when one of its merges has a token id the encoder does not
 * hold (the list keeps that merge: fromJSON replaces the list).  A text with such an id replays alone.
 * Any other failure (a device fault, out of memory) is reported once as a process warning and not
 * remembered: that call replays, and the next one tries the device again with its encoder rebuilt.
 */
const CAPABILITY_LIST = /merge token id out of range|more merges than token ids/
const CAPABILITY_TEXT = /token id out of range in text/
let warned = false
function encodeIdsMaybeOnDevice(owner, list, tripleOf, ids) {
  if (!encodeOnDevice(ids.length, list.length)) return null
  if (ENCODE_DEVICE !== '1' && (owner._enc_failed === true || owner._enc_failed === list))
    return null
  try {
    return encodeIdsOnDevice(owner, list, tripleOf, ids)
  } catch (e) {
    if (ENCODE_DEVICE === '1') throw e
    if (!Object.prototype.hasOwnProperty.call(owner, '_enc_failed'))
      Object.defineProperty(owner, '_enc_failed', { value: null, writable: true, enumerable: false })
    let msg = String((e && e.message) || e)
    if (!owner._encoder) {
      owner._enc_failed = true
    } else {
      // (the encoder may hold part of the list: the next call loads it again from the start)
      owner._enc_list = null
      if (CAPABILITY_LIST.test(msg)) owner._enc_failed = list
      else if (!CAPABILITY_TEXT.test(msg) && !warned) {
        warned = true
        process.emitWarning('bpe device encoder failed, this call replays the merges in JS: ' + msg)
      }
    }
    return null
  }
}

/**
 * The owner's device decoder (bpe_decoder_*), holding the chars of `owner.token_table` in id order
 * and `owner.from_vector_index`; the tokens added to the table since the last call are appended to
 * it (addToCorpus, applyMerge, restoreMerge, mergeUntil), a replaced or shortened table (fromJSON)
 * rebuilds it, and a new from_vector_index array (compactVectorIndex makes one each time) is sent
 * again.  The owner keeps the handle in non-enumerable fields.
 */
function syncDecoder(owner) {
  let n = loadNativeDecode()
  let table = owner.token_table
  if (!owner._decoder) {
    for (let k of ['_decoder', '_dec_table', '_dec_n', '_dec_last', '_dec_index'])
      if (!Object.prototype.hasOwnProperty.call(owner, k))
        Object.defineProperty(owner, k, { value: null, writable: true, enumerable: false })
    owner._decoder = n.createDecoder(0)
    owner._dec_table = null
  }
  let have = owner._dec_n || 0
  if (owner._dec_table !== table || have > table.length || (have && table[have - 1] !== owner._dec_last)) {
    n.decoderClear(owner._decoder)
    owner._dec_table = table
    owner._dec_index = null
    owner._dec_n = have = 0
  }
  if (have < table.length) {
    let k = table.length - have
    let off = new Float64Array(k + 1)
    for (let i = 0; i < k; i++) off[i + 1] = off[i] + table[have + i].chars.length
    let units = new Uint16Array(off[k])
    for (let i = 0; i < k; i++) {
      let chars = table[have + i].chars
      for (let j = 0, p = off[i]; j < chars.length; j++) units[p + j] = chars.charCodeAt(j)
    }
    owner._dec_n = 0 // (a failed append leaves the decoder to be rebuilt)
    owner._dec_table = null
    n.decoderAddTokens(owner._decoder, units, off)
    owner._dec_table = table
    owner._dec_index = null // (new tokens drop the decoder's index, core.ts:348)
  }
  owner._dec_n = table.length
  owner._dec_last = table.length ? table[table.length - 1] : null
  if (owner._dec_index !== owner.from_vector_index) {
    n.decoderSetVectorIndex(owner._decoder, owner.from_vector_index ? Int32Array.from(owner.from_vector_index) : null)
    owner._dec_index = owner.from_vector_index
  }
  return owner._decoder
}

/** a batch of vectors (Int32Array values, Float64Array offsets) through the owner's decoder -> strings */
function decodeVectorsOnDevice(owner, vals, off) {
  return loadNativeDecode().decodeBatch(syncDecoder(owner), vals, off, 1)
}

/** ... as UTF-8 bytes, encoded on the device as Buffer.from(text) encodes them -> Buffer[] */
function decodeVectorsUtf8OnDevice(owner, vals, off) {
  return loadNativeUtf8Out().decodeUtf8Batch(syncDecoder(owner), vals, off, 1)
}

/**
 * The owner's device text encoder (bpe_encode_text_batch: chars -> ids -> merges -> vector indices,
 * all on the device), following the owner's tables: the merges appended to `list` since the last
 * call are appended (a replaced or shortened list rebuilds them), the char table is sent again when
 * `owner.char_to_token` has gained keys or been replaced (keys that are not exactly one code point
 * are skipped: `for (let char of content)` never produces them), and the index when
 * `owner.to_vector_index` is a new array (compactVectorIndex makes one each time; holes go as -1).
 * The owner keeps the handle in non-enumerable fields.
 */
function syncTextEncoder(owner, list, tripleOf) {
  let n = loadNativeText()
  list = list || owner.merge_tokens
  tripleOf = tripleOf || (m => [m[0].index, m[1].index, m[2].index])
  if (!owner._tenc) {
    for (let k of ['_tenc', '_tenc_list', '_tenc_n', '_tenc_last', '_tenc_chars', '_tenc_nchars', '_tenc_index'])
      if (!Object.prototype.hasOwnProperty.call(owner, k))
        Object.defineProperty(owner, k, { value: null, writable: true, enumerable: false })
    owner._tenc = n.createTextEncoder(0)
    owner._tenc_list = null
  }
  let have = owner._tenc_n || 0
  if (owner._tenc_list !== list || have > list.length || (have && list[have - 1] !== owner._tenc_last)) {
    n.textEncoderClear(owner._tenc)
    owner._tenc_list = list
    owner._tenc_index = null // (clear drops the encoder's index, core.ts:348)
    owner._tenc_n = have = 0
  }
  if (have < list.length) {
    let k = list.length - have
    let abc = new Int32Array(3 * k)
    for (let i = 0; i < k; i++) {
      let t = tripleOf(list[have + i])
      abc[3 * i] = t[0]
      abc[3 * i + 1] = t[1]
      abc[3 * i + 2] = t[2]
    }
    owner._tenc_n = 0 // (a failed append leaves the merges to be rebuilt)
    owner._tenc_list = null
    n.textEncoderAddMerges(owner._tenc, abc)
    owner._tenc_list = list
    owner._tenc_index = null // (new merges drop the encoder's index)
  }
  owner._tenc_n = list.length
  owner._tenc_last = list.length ? list[list.length - 1] : null
  let table = owner.char_to_token
  let keys = Object.keys(table)
  if (owner._tenc_chars !== table || owner._tenc_nchars !== keys.length) {
    let cps = new Uint32Array(keys.length)
    let ids = new Int32Array(keys.length)
    let m = 0
    for (let key of keys) {
      let cp = key.codePointAt(0)
      if (cp === undefined || key.length !== (cp > 0xffff ? 2 : 1)) continue
      cps[m] = cp
      ids[m++] = table[key].index
    }
    owner._tenc_chars = null
    n.textEncoderSetChars(owner._tenc, cps.subarray(0, m), ids.subarray(0, m))
    owner._tenc_chars = table
    owner._tenc_nchars = keys.length
  }
  if (owner._tenc_index !== owner.to_vector_index) {
    let index = null
    if (owner.to_vector_index) {
      index = new Int32Array(owner.to_vector_index.length).fill(-1)
      owner.to_vector_index.forEach((v, i) => {
        index[i] = v
      })
    }
    n.textEncoderSetVectorIndex(owner._tenc, index)
    owner._tenc_index = owner.to_vector_index
  }
  return owner._tenc
}

/** texts (strings) as one Uint16Array of UTF-16 units and a Float64Array of offsets */
function textsToUnits(texts) {
  let off = new Float64Array(texts.length + 1)
  for (let k = 0; k < texts.length; k++) off[k + 1] = off[k] + texts[k].length
  // (one conversion for the batch; 'utf16le' writes the code units as they are, lone surrogates too)
  let buf = Buffer.from(texts.join(''), 'utf16le')
  if (buf.byteOffset & 1) buf = Buffer.from(new Uint8Array(buf))
  return [new Uint16Array(buf.buffer, buf.byteOffset, buf.length >> 1), off]
}

/** buffers (Buffer / Uint8Array, UTF-8) as one Uint8Array of bytes and a Float64Array of offsets */
function buffersToBytes(buffers) {
  let off = new Float64Array(buffers.length + 1)
  for (let k = 0; k < buffers.length; k++) off[k + 1] = off[k] + buffers[k].length
  let bytes = new Uint8Array(off[buffers.length])
  for (let k = 0; k < buffers.length; k++) bytes.set(buffers[k], off[k])
  return [bytes, off]
}

/**
 * A batch of texts through the owner's device text encoder -> array of vectors, or null when the
 * device cannot take the call (the caller then maps encodeToVector in JS): BPE_ENCODE_DEVICE=0, no
 * addon or no HIP device (remembered for the owner's lifetime), or a token id the device does not
 * hold (>= BPE_MAX_VOCAB: remembered while the owner keeps that merge list and char table).  With
 * BPE_ENCODE_DEVICE=1 the device's errors go through.  The reference's own errors (an unknown char,
 * an unknown token index) are thrown with its strings either way.
 * utf8: `texts` are Buffers / Uint8Arrays of UTF-8 bytes, decoded on the device (bpe_encode_utf8_batch).
 */
const CAPABILITY_TEXT_TABLE = /merge token id out of range|more merges than token ids|char token id out of range/
function encodeTextsMaybeOnDevice(owner, list, tripleOf, texts, utf8) {
  if (ENCODE_DEVICE === '0') return null
  if (
    ENCODE_DEVICE !== '1' &&
    (owner._tenc_failed === true || (owner._tenc_failed && owner._tenc_failed === list))
  )
    return null
  let res
  try {
    let enc = syncTextEncoder(owner, list, tripleOf)
    if (utf8) {
      let [bytes, off] = buffersToBytes(texts)
      res = loadNativeUtf8().encodeUtf8Batch(enc, bytes, off, 1)
    } else {
      let [units, off] = textsToUnits(texts)
      res = loadNativeText().encodeTextBatch(enc, units, off, 1)
    }
  } catch (e) {
    let msg = String((e && e.message) || e)
    let m = /^unknown token, char: U\+([0-9A-F]+) \(text \d+, unit \d+\)$/.exec(msg)
    if (m) throw new Error('unknown token, char: ' + JSON.stringify(String.fromCodePoint(parseInt(m[1], 16))))
    m = /^unknown token index: (-?\d+) \(text \d+, position \d+\)$/.exec(msg)
    if (m) throw new Error(`unknown token index: ${m[1]}`)
    if (ENCODE_DEVICE === '1') throw e
    if (!Object.prototype.hasOwnProperty.call(owner, '_tenc_failed'))
      Object.defineProperty(owner, '_tenc_failed', { value: null, writable: true, enumerable: false })
    if (!owner._tenc) {
      owner._tenc_failed = true
    } else {
      // (the encoder may hold part of the tables: the next call loads them again from the start)
      owner._tenc_list = null
      owner._tenc_chars = null
      if (CAPABILITY_TEXT_TABLE.test(msg)) owner._tenc_failed = list
      else if (!warned) {
        warned = true
        process.emitWarning('bpe device text encoder failed, this call encodes in JS: ' + msg)
      }
    }
    return null
  }
  let [vals, off] = res
  let out = new Array(texts.length)
  for (let k = 0; k < texts.length; k++) out[k] = Array.from(vals.subarray(off[k], off[k + 1]))
  return out
}

/**
 * A batch of texts through the owner's device text encoder straight into the engine's corpus
 * (bpe_restore_text_batch: encodeToCode on the device, then every text one sample) -> true, or false
 * when the device cannot take the call (the caller then loops restoreToCorpus), under
 * encodeTextsMaybeOnDevice's rules: BPE_ENCODE_DEVICE=0, no addon or no HIP device, a token id the
 * device does not hold; with BPE_ENCODE_DEVICE=1 the device's errors go through.  The reference's
 * `unknown token, char: "x"` is thrown with its string either way; the batch is atomic, so no text has
 * been added then (the reference's loop would have added the texts before the failing one).
 * utf8: `texts` are Buffers / Uint8Arrays of UTF-8 bytes, decoded on the device (bpe_restore_utf8_batch).
 * lines (a BPE_LINES_* mode, or undefined): the texts are split into samples by that corpus helper on
 * the device first (bpe_restore_lines_batch, bpe_restore_lines_utf8_batch).
 */
function restoreTextsMaybeOnDevice(owner, engine, list, tripleOf, texts, utf8, lines) {
  if (ENCODE_DEVICE === '0') return false
  if (
    ENCODE_DEVICE !== '1' &&
    (owner._tenc_failed === true || (owner._tenc_failed && owner._tenc_failed === list))
  )
    return false
  try {
    let enc = syncTextEncoder(owner, list, tripleOf)
    if (utf8) {
      let [bytes, off] = buffersToBytes(texts)
      if (lines === undefined) loadNativeUtf8().restoreUtf8Batch(engine, enc, bytes, off)
      else loadNativeLines().restoreLinesUtf8Batch(engine, enc, lines, bytes, off)
    } else {
      let [units, off] = textsToUnits(texts)
      if (lines === undefined) loadNativeRestore().restoreTextBatch(engine, enc, units, off)
      else loadNativeLines().restoreLinesBatch(engine, enc, lines, units, off)
    }
  } catch (e) {
    let msg = String((e && e.message) || e)
    let m = /^unknown token, char: U\+([0-9A-F]+) \(text \d+, unit \d+\)$/.exec(msg)
    if (m) throw new Error('unknown token, char: ' + JSON.stringify(String.fromCodePoint(parseInt(m[1], 16))))
    if (ENCODE_DEVICE === '1') throw e
    if (!Object.prototype.hasOwnProperty.call(owner, '_tenc_failed'))
      Object.defineProperty(owner, '_tenc_failed', { value: null, writable: true, enumerable: false })
    if (!owner._tenc) {
      owner._tenc_failed = true
    } else {
      // (the encoder may hold part of the tables: the next call loads them again from the start)
      owner._tenc_list = null
      owner._tenc_chars = null
      if (CAPABILITY_TEXT_TABLE.test(msg)) owner._tenc_failed = list
      else if (!warned) {
        warned = true
        process.emitWarning('bpe device restore failed, this call restores text by text in JS: ' + msg)
      }
    }
    return false
  }
  return true
}

/**
 * The engine's char table (bpe_set_chars) follows `owner.char_to_token`: sent whole when the object
 * was replaced (fromJSON), when the engine is new, or when it has gained keys the engine did not make
 * itself (addToCorpus maps chars on the host and does not feed the table).  addToCorpusBatch counts
 * the chars the engine numbered (`owner._eng_nchars`).  Keys that are not exactly one code point are
 * skipped, as syncTextEncoder skips them.
 */
function syncEngineChars(owner, engine) {
  for (let k of ['_eng_chars', '_eng_nchars', '_eng_for'])
    if (!Object.prototype.hasOwnProperty.call(owner, k))
      Object.defineProperty(owner, k, { value: null, writable: true, enumerable: false })
  let table = owner.char_to_token
  let keys = Object.keys(table)
  if (owner._eng_for === engine && owner._eng_chars === table && owner._eng_nchars === keys.length) return
  let cps = new Uint32Array(keys.length)
  let ids = new Int32Array(keys.length)
  let m = 0
  for (let key of keys) {
    let cp = key.codePointAt(0)
    if (cp === undefined || key.length !== (cp > 0xffff ? 2 : 1)) continue
    cps[m] = cp
    ids[m++] = table[key].index
  }
  owner._eng_chars = null
  loadNativeIngest().setChars(engine, cps.subarray(0, m), ids.subarray(0, m))
  owner._eng_for = engine
  owner._eng_chars = table
  owner._eng_nchars = keys.length
}

/**
 * The export's addon, or null when the callers are to take their JS route: BPE_ENCODE_DEVICE=0, or the
 * addon is not built (with BPE_ENCODE_DEVICE=1 that is an error).
 */
function exportAddon() {
  if (ENCODE_DEVICE === '0' || nativeExportMissing) return null
  try {
    return loadNativeExport()
  } catch (e) {
    if (ENCODE_DEVICE === '1') throw e
    nativeExportMissing = true
    return null
  }
}

/** BPE_EXPORT_* (include/bpe.h) */
const EXPORT_IDS = 0
const EXPORT_VECTORS = 1
const EXPORT_CODE = 2

/** sample indices for the export's addon: null (every sample) or a Float64Array */
function exportIndices(indices) {
  return indices === undefined || indices === null ? null : Float64Array.from(indices)
}

/**
 * The code strings (`corpus_in_code` / `content_code`: unit = token index + 1) of the samples
 * `indices` (null: every sample) from the device's code form, each string made from its UTF-16 units
 * in one call -> string[], or null when there is no addon to ask (exportAddon).
 */
function corpusCodesOnDevice(engine, indices) {
  let addon = exportAddon()
  if (!addon) return null
  let [units, off] = addon.exportSamples(engine, EXPORT_CODE, exportIndices(indices), null)
  let buf = Buffer.from(units.buffer, units.byteOffset, units.byteLength)
  let out = new Array(off.length - 1)
  for (let s = 0; s + 1 < off.length; s++) out[s] = buf.toString('utf16le', 2 * off[s], 2 * off[s + 1])
  return out
}

/**
 * The samples `indices` (null: every sample) as vectors through `owner.to_vector_index` (holes go as
 * -1) -> Int32Array[], or null when there is no addon to ask.  The device's `unknown token index: N
 * (sample K, position I)` is thrown as the reference's `unknown token index: N`.
 */
function corpusVectorsOnDevice(owner, engine, indices) {
  let addon = exportAddon()
  if (!addon) return null
  let index = new Int32Array(owner.to_vector_index.length).fill(-1)
  owner.to_vector_index.forEach((v, i) => {
    index[i] = v
  })
  let vals, off
  try {
    ;[vals, off] = addon.exportSamples(engine, EXPORT_VECTORS, exportIndices(indices), index)
  } catch (e) {
    let m = /^unknown token index: (\d+) \(sample \d+, position \d+\)$/.exec(String(e && e.message))
    if (m) throw new Error(`unknown token index: ${m[1]}`)
    throw e
  }
  let out = new Array(off.length - 1)
  for (let s = 0; s + 1 < off.length; s++) out[s] = vals.slice(off[s], off[s + 1])
  return out
}

/** the samples `indices` (null: every sample) as text through the owner's device decoder, or null */
function corpusTextsOnDevice(owner, engine, indices) {
  let addon = exportAddon()
  if (!addon) return null
  return addon.exportText(engine, syncDecoder(owner), exportIndices(indices))
}

/** ... as UTF-8 bytes (bpe_export_utf8_batch) -> Buffer[], or null when there is no addon to ask */
function corpusTextsUtf8OnDevice(owner, engine, indices) {
  if (!exportAddon()) return null
  let addon
  try {
    addon = loadNativeUtf8Out()
  } catch (e) {
    if (ENCODE_DEVICE === '1') throw e
    return null
  }
  return addon.exportUtf8(engine, syncDecoder(owner), exportIndices(indices))
}

/** BPE_SKIPGRAM_MAX_WINDOW (include/bpe.h) */
const SKIPGRAM_MAX_WINDOW = 64

/** the window of a skip-gram call: an integer in [1, SKIPGRAM_MAX_WINDOW], 2 when left out */
function skipGramWindow(window) {
  if (window === undefined) return 2
  if (!Number.isInteger(window) || window < 1 || window > SKIPGRAM_MAX_WINDOW)
    throw new RangeError(`skip-gram window ${window} outside [1, ${SKIPGRAM_MAX_WINDOW}]`)
  return window
}

/**
 * Vectors (one array per text) -> their (target, context) pairs over `window` values on each side, in
 * JS: for every value of a text in order, its neighbours from `window` before to `window` after it,
 * in order, without itself and without places outside the text.  What the device forms compute; the
 * route of a call the device cannot take.
 */
function expandSkipGram(vectors, window) {
  let offsets = new Float64Array(vectors.length + 1)
  vectors.forEach((v, k) => {
    let n = v.length
    offsets[k + 1] = offsets[k] + (n <= 1 ? 0 : n <= window + 1 ? n * (n - 1) : window * (2 * n - window - 1))
  })
  let targets = new Int32Array(offsets[vectors.length])
  let contexts = new Int32Array(offsets[vectors.length])
  let p = 0
  for (let v of vectors) {
    for (let i = 0; i < v.length; i++) {
      let last = Math.min(i + window, v.length - 1)
      for (let j = Math.max(i - window, 0); j <= last; j++) {
        if (j === i) continue
        targets[p] = v[i]
        contexts[p++] = v[j]
      }
    }
  }
  return { targets, contexts, offsets }
}

/**
 * A batch of texts through the owner's device text encoder and the skip-gram expansion behind it
 * (bpe_skipgram_text_batch; utf8: Buffers / Uint8Arrays through bpe_skipgram_utf8_batch) ->
 * {targets, contexts, offsets}, or null when the device cannot take the call (the caller then expands
 * encodeToVectorBatch's vectors in JS, which settles what the device can do under its own rules).  The
 * reference's own errors are thrown with its strings; with BPE_ENCODE_DEVICE=1 the device's go through.
 */
function skipGramTextsMaybeOnDevice(owner, list, tripleOf, texts, window, utf8) {
  if (ENCODE_DEVICE === '0') return null
  if (
    ENCODE_DEVICE !== '1' &&
    (owner._tenc_failed === true || (owner._tenc_failed && owner._tenc_failed === list))
  )
    return null
  try {
    let addon = loadNativeSkipGram()
    let enc = syncTextEncoder(owner, list, tripleOf)
    let [data, off] = utf8 ? buffersToBytes(texts) : textsToUnits(texts)
    let res = utf8 ? addon.skipGramUtf8Batch(enc, data, off, window, 1) : addon.skipGramTextBatch(enc, data, off, window, 1)
    return { targets: res[0], contexts: res[1], offsets: res[2] }
  } catch (e) {
    let msg = String((e && e.message) || e)
    let m = /^unknown token, char: U\+([0-9A-F]+) \(text \d+, unit \d+\)$/.exec(msg)
    if (m) throw new Error('unknown token, char: ' + JSON.stringify(String.fromCodePoint(parseInt(m[1], 16))))
    m = /^unknown token index: (-?\d+) \(text \d+, position \d+\)$/.exec(msg)
    if (m) throw new Error(`unknown token index: ${m[1]}`)
    if (ENCODE_DEVICE === '1') throw e
    return null
  }
}

/**
 * The samples `indices` (null: every sample) as skip-gram pairs of their vectors through
 * `owner.to_vector_index` (bpe_export_skipgram) -> {targets, contexts, offsets}, or null when there is
 * no addon to ask.  The device's `unknown token index: N (sample K, position I)` is thrown as the
 * reference's `unknown token index: N`.
 */
function corpusSkipGramOnDevice(owner, engine, indices, window) {
  if (!exportAddon()) return null
  let addon
  try {
    addon = loadNativeSkipGram()
  } catch (e) {
    if (ENCODE_DEVICE === '1') throw e
    return null
  }
  let index = new Int32Array(owner.to_vector_index.length).fill(-1)
  owner.to_vector_index.forEach((v, i) => {
    index[i] = v
  })
  try {
    let res = addon.exportSkipGram(engine, EXPORT_VECTORS, exportIndices(indices), index, window)
    return { targets: res[0], contexts: res[1], offsets: res[2] }
  } catch (e) {
    let m = /^unknown token index: (\d+) \(sample \d+, position \d+\)$/.exec(String(e && e.message))
    if (m) throw new Error(`unknown token index: ${m[1]}`)
    throw e
  }
}

/** engine ids -> code point string (code = index + 1, core.ts:149) */
function idsToCode(ids, begin, end) {
  let parts = []
  for (let i = begin; i < end; i += 8192) {
    let part = []
    let stop = Math.min(end, i + 8192)
    for (let j = i; j < stop; j++) part.push(ids[j] + 1)
    parts.push(String.fromCodePoint.apply(null, part))
  }
  return parts.join('')
}

/** JS `x || fallback` for numeric options, mapped onto the C ABI's int64 conventions. */
function maxLengthArg(max_length) {
  // core.ts:255,272: falsy -> unlimited; otherwise `len <= max_length`
  if (!max_length) return 0
  if (max_length === Infinity) return 0
  if (max_length === -Infinity) return -1
  let v = Math.floor(max_length) // integer lengths: len <= x  <=>  len <= floor(x)
  return v === 0 ? -1 : v // 0 < x < 1: nothing fits, but 0 means "unlimited" in the C ABI
}

function minWeightArg(options) {
  // core.ts:256: options?.min_weight || 2 ; core.ts:313: W < min_weight -> null
  let min_weight = (options && options.min_weight) || 2
  if (min_weight === Infinity) return Number.MAX_SAFE_INTEGER
  if (min_weight === -Infinity) return -Number.MAX_SAFE_INTEGER
  let v = Math.ceil(min_weight) // integer W: W < x  <=>  W < ceil(x)
  return v === 0 ? -1 : v // 0 would mean "default" in the C ABI; W >= 1 always passes -1
}

module.exports = {
  loadNative,
  loadNativeDecode,
  loadNativeText,
  loadNativeIngest,
  loadNativeRestore,
  loadNativeUtf8,
  loadNativeUtf8Out,
  loadNativeLines,
  linesMode,
  buffersToBytes,
  maxLengthArg,
  minWeightArg,
  encodeOnDevice,
  encodeIdsOnDevice,
  encodeIdsMaybeOnDevice,
  syncDecoder,
  decodeVectorsOnDevice,
  decodeVectorsUtf8OnDevice,
  syncTextEncoder,
  encodeTextsMaybeOnDevice,
  restoreTextsMaybeOnDevice,
  textsToUnits,
  syncEngineChars,
  idsToCode,
  loadNativeExport,
  corpusCodesOnDevice,
  corpusVectorsOnDevice,
  corpusTextsOnDevice,
  corpusTextsUtf8OnDevice,
  loadNativeSkipGram,
  skipGramWindow,
  expandSkipGram,
  skipGramTextsMaybeOnDevice,
  corpusSkipGramOnDevice,
}
