// BPETokenizer.encodeToVectorBatch (js/core.js over addon/bpe_text_napi.node, bpe_encode_text_batch
// on the GPU; BPE_ENCODE_DEVICE=1, so nothing falls back) against the reference's own loop,
// encodeToVector (core.ts:424-445), mapped over the batch: on BASELINE config 2, on 50 of the small
// golden cases, after fromJSON, after further applyMerge calls and after addToCorpus of new chars,
// on both error strings, and back through decodeVectorBatch.
// Run: BPE_ENCODE_DEVICE=1 node tests/js/text_encoder_gpu.js
'use strict'
const assert = require('assert')
const path = require('path')
const fs = require('fs')
assert.strictEqual(process.env.BPE_ENCODE_DEVICE, '1')
const { BPETokenizer } = require(path.join(__dirname, '..', '..', 'bpe-tokenizer_amd', 'js', 'core.js'))

function sameAsMapped(t, texts, what) {
  const got = t.encodeToVectorBatch(texts)
  const want = texts.map(s => t.encodeToVector(s))
  assert.deepStrictEqual(got, want, what)
  return got
}

function messageOf(fn) {
  try {
    fn()
  } catch (e) {
    return e.message
  }
  return null
}

function sameError(t, batch, re) {
  const want = messageOf(() => batch.map(s => t.encodeToVector(s)))
  assert.ok(re.test(want), want)
  assert.strictEqual(messageOf(() => t.encodeToVectorBatch(batch)), want, JSON.stringify(batch))
}

// ---- config 2 ---------------------------------------------------------------------------------
const g = JSON.parse(fs.readFileSync(path.join(__dirname, '..', 'golden', 'config2.json')))
function xorshiftCodes(seed, A, base, n) {
  const out = new Uint16Array(n)
  let x = seed >>> 0
  for (let i = 0; i < n; i++) {
    x ^= x << 13; x >>>= 0
    x ^= x >>> 17
    x ^= x << 5; x >>>= 0
    out[i] = base + Math.floor(x * A / 4294967296)
  }
  return out
}
const codes = xorshiftCodes(g.seed, g.A, g.base, g.total)
const samples = []
for (let off = 0; off < g.total; off += g.sample) {
  const part = codes.subarray(off, Math.min(g.total, off + g.sample))
  let s = ''
  for (let i = 0; i < part.length; i += 8192) s += String.fromCharCode.apply(null, part.subarray(i, i + 8192))
  samples.push(s)
}
const big = new BPETokenizer()
for (const s of samples) big.addToCorpus(s)
big.mergeUntil({ min_weight: g.min_weight, max_iterations: g.max_iterations })
assert.deepStrictEqual(big.merge_tokens.map(([a, b, c]) => [a.index, b.index, c.original_weight]), g.merges)
// the samples cut into serving-size texts (the merge-rank route), and two whole samples (replay)
const texts2 = []
for (const s of samples) for (let i = 0; i < s.length; i += 4000) texts2.push(s.slice(i, i + 4000))
const t0 = Date.now()
const vectors2 = big.encodeToVectorBatch(texts2)
const config2_s = (Date.now() - t0) / 1000
for (let i = 0; i < texts2.length; i += 97) assert.deepStrictEqual(vectors2[i], big.encodeToVector(texts2[i]), 'config2 text ' + i)
sameAsMapped(big, samples.slice(0, 2).concat(['', texts2[1]]), 'config2 whole samples')
assert.ok(!Object.keys(big).some(k => k.startsWith('_tenc')), 'text encoder fields are not enumerable')
const back = big.decodeVectorBatch(vectors2)
for (let i = 0; i < texts2.length; i++) assert.ok(back[i] === texts2[i], 'config2 round trip ' + i)

// ---- 50 small cases ------------------------------------------------------------------------------
const golden = JSON.parse(fs.readFileSync(path.join(__dirname, '..', 'golden', 'small_cases.json')))
let n_cases = 0, n_texts = 0
const step = Math.floor(golden.cases.length / 50)
let last = null
for (let k = 0; k < golden.cases.length && n_cases < 50; k += step) {
  const c = golden.cases[k]
  if (!c.samples.some(s => s.length)) continue
  const t = new BPETokenizer()
  for (const s of c.samples) t.addToCorpus(s)
  const o = {}
  for (const key in c.opts) if (c.opts[key] !== null) o[key] = c.opts[key]
  t.mergeUntil(o)
  const keep = c.samples.filter((s, i) => typeof c.vectors[i] !== 'string')
  const got = sameAsMapped(t, keep, c.name)
  assert.deepStrictEqual(got, c.vectors.filter(v => typeof v !== 'string'), c.name)
  assert.deepStrictEqual(t.decodeVectorBatch(got), keep, c.name)
  n_texts += keep.length
  n_cases++
  last = { t, keep }
}
assert.ok(n_cases >= 45 && n_texts >= 100, n_cases + ' cases, ' + n_texts + ' texts')

// ---- the encoder follows the tokenizer ---------------------------------------------------------------
const t = last.t
// addToCorpus of new chars: the char table is sent again (the old index stays, as in the reference)
t.addToCorpus('\u{1F600}\ud800 zebra \u{1F600}\u{1F600}\ud800 zebra')
t.compactVectorIndex()
sameAsMapped(t, last.keep.concat(['\u{1F600}\ud800 z', 'zebra', '']), 'after addToCorpus')
// further applyMerge calls: the merges are appended and the index rebuilt
for (let i = 0; i < 3; i++) {
  const m = t.findNextMerge({ min_weight: 2 })
  assert.ok(m)
  t.applyMerge(m)
}
assert.strictEqual(t.to_vector_index, null)
const texts = ['\u{1F600}\u{1F600}\ud800 zebra', ' zebra zebra', '\u{1F600}\ud800 zebra \u{1F600}\u{1F600}\ud800 zebra']
const vecs = sameAsMapped(t, texts, 'after more merges')
assert.deepStrictEqual(t.decodeVectorBatch(vecs), texts)
// (a char whose every occurrence the new merges took is a hole now: the same outcome either way)
for (const s of ['\ud800', 'z', '\u{1F600}', ' ']) {
  const want = messageOf(() => t.encodeToVector(s))
  assert.strictEqual(messageOf(() => t.encodeToVectorBatch(['zebra', s])), want, JSON.stringify(s))
  if (want === null) assert.deepStrictEqual(t.encodeToVectorBatch(['zebra', s])[1], t.encodeToVector(s))
}
// both error strings, identical to the JS loop's
sameError(t, ['zebra', 'zebra\u2603'], /^unknown token, char: "\u2603"$/)
sameError(t, ['\u{1F600}', 'ze\u{1F601}bra', '\u2603'], /^unknown token, char: /)
sameError(t, ['ze\udc00'], /^unknown token, char: "\\udc00"$/)
// fromJSON of another tokenizer: merges, chars and index are rebuilt from the new tables
t.fromJSON(JSON.parse(JSON.stringify(big.toJSON())))
sameAsMapped(t, texts2.slice(0, 40), 'after fromJSON')
// and a small one with a hole (a char token whose every occurrence was merged away)
t.fromJSON({ version: 2, char_count: 3, token_table: [['a', 2, 2], ['b', 0, 1], ['\u{1F600}', 1, 1], ['a\u{1F600}', 1, 1]],
             merge_codes: [['\u0001', '\u0003', '\u0004']] })
assert.deepStrictEqual(t.encodeToVectorBatch(['a', '', 'a\u{1F600}a']), [[0], [], [2, 0]])
sameError(t, ['a', 'ab', 'z'], /^unknown token index: 1$/)
sameError(t, ['z', 'b'], /^unknown token, char: "z"$/)
sameError(t, ['bz'], /^unknown token, char: "z"$/)
assert.deepStrictEqual(t.encodeToVectorBatch([]), [])
assert.strictEqual(messageOf(() => new BPETokenizer().encodeToVectorBatch(['a'])),
                   'token table is empty, have you called tokenizer.addToCorpus()?')
assert.ok(!Object.keys(t).some(k => k.startsWith('_tenc')), 'text encoder fields are not enumerable')

console.log('text_encoder_gpu ok', JSON.stringify({ cases: n_cases, texts: n_texts, config2_texts: texts2.length, config2_s }))
