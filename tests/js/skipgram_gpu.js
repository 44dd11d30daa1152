// BPETokenizer.skipGramBatch / skipGramBatchUtf8 / corpusToSkipGramBatch (js/core.js over
// addon/bpe_skipgram_napi.node: encoded and expanded on the GPU) against the same class's
// encodeToVector per text, expanded by the rule restated below, on a golden case
// (tests/golden/small_cases.json) and on texts of several scripts, an empty text and one-char texts.
// Run: node tests/js/skipgram_gpu.js
'use strict'
const assert = require('assert')
const path = require('path')
const fs = require('fs')
const { BPETokenizer } = require(path.join(__dirname, '..', '..', 'bpe-tokenizer_amd', 'js', 'core.js'))
const native = require(path.join(__dirname, '..', '..', 'bpe-tokenizer_amd', 'js', 'native.js'))

// whether the batches went through the native calls
const calls = { skipGramTextBatch: 0, skipGramUtf8Batch: 0, exportSkipGram: 0 }
const addon = native.loadNativeSkipGram()
for (const name of Object.keys(calls)) {
  const inner = addon[name]
  addon[name] = function () {
    calls[name]++
    return inner.apply(this, arguments)
  }
}

// the rule, per token: token i's contexts are the places i - w .. i + w in order, without the places
// before the text, i itself, and the places past the text
function rule(vectors, w) {
  const targets = [], contexts = [], offsets = [0]
  for (const v of vectors) {
    for (let i = 0; i < v.length; i++)
      for (let d = -w; d <= w; d++) {
        if (d === 0 || i + d < 0 || i + d >= v.length) continue
        targets.push(v[i])
        contexts.push(v[i + d])
      }
    offsets.push(targets.length)
  }
  return { targets, contexts, offsets }
}

function same(got, vectors, w, what) {
  const want = rule(vectors, w)
  assert(got.targets instanceof Int32Array && got.contexts instanceof Int32Array, what + ': Int32Array planes')
  assert.deepStrictEqual(Array.from(got.offsets), want.offsets, what + ': offsets')
  assert.deepStrictEqual(Array.from(got.targets), want.targets, what + ': targets')
  assert.deepStrictEqual(Array.from(got.contexts), want.contexts, what + ': contexts')
}

function outcome(fn) {
  try {
    return fn()
  } catch (e) {
    return 'error: ' + e.message
  }
}

// ---- a golden case: its samples, trained as the case says ----
const cases = JSON.parse(fs.readFileSync(path.join(__dirname, '..', 'golden', 'small_cases.json'))).cases
const g = cases.find(c => c.merges.length >= 20 && c.samples.length >= 3 && c.vectors.every(v => Array.isArray(v)))
const t = new BPETokenizer()
for (const s of g.samples) t.addToCorpus(s)
t.mergeUntil(g.opts)
t.compactVectorIndex()
const texts = g.samples.concat(['', g.samples[0].slice(0, 1), g.samples[1].repeat(30)])
const vectors = texts.map(s => Array.from(t.encodeToVector(s)))
assert.deepStrictEqual(vectors.slice(0, g.samples.length), g.vectors)
for (const w of [1, 2, 3, 5, 64]) {
  same(t.skipGramBatch(texts, w), vectors, w, 'texts, window ' + w)
  same(t.skipGramBatchUtf8(texts.map(s => Buffer.from(s)), w), vectors, w, 'buffers, window ' + w)
}
// the default window is 2
same(t.skipGramBatch(texts), vectors, 2, 'texts, default window')
same(t.skipGramBatchUtf8(texts.map(s => Buffer.from(s))), vectors, 2, 'buffers, default window')
same(t.skipGramBatchUtf8([new Uint8Array(Buffer.from(texts[0]))]), [vectors[0]], 2, 'a Uint8Array')
assert(t.skipGramBatch(texts).targets.length > 200)

// ---- the corpus: every sample, chosen samples, repeats ----
const corpus = t.corpusToVectorBatch().map(v => Array.from(v))
assert.deepStrictEqual(corpus, g.vectors)
same(t.corpusToSkipGramBatch(), corpus, 2, 'corpus, default window')
same(t.corpusToSkipGramBatch(null, 5), corpus, 5, 'corpus, window 5')
same(t.corpusToSkipGramBatch(undefined, 1), corpus, 1, 'corpus, window 1')
const pick = [g.samples.length - 1, 0, 0, 1]
same(t.corpusToSkipGramBatch(pick, 3), pick.map(k => corpus[k]), 3, 'chosen samples')
same(t.corpusToSkipGramBatch([]), [], 2, 'no sample')
same(t.skipGramBatch([]), [], 2, 'no text')
same(new BPETokenizer().corpusToSkipGramBatch(), [], 2, 'no corpus')

// ---- several scripts, surrogate pairs, after a few merges ----
const mixed = ['Съешь ещё этих мягких булок 色は匂へど 😀🎉 naïve', '', 'a', 'ab', 'abc'.repeat(2000), '😀']
const u = new BPETokenizer()
for (const s of mixed) u.addToCorpus(s)
u.mergeUntil({ min_weight: 2, max_iterations: 8 })
u.compactVectorIndex()
const uv = mixed.map(s => Array.from(u.encodeToVector(s)))
same(u.skipGramBatch(mixed, 2), uv, 2, 'mixed texts')
same(u.skipGramBatchUtf8(mixed.map(s => Buffer.from(s)), 4), uv, 4, 'mixed buffers')
same(u.corpusToSkipGramBatch(null, 2), uv, 2, 'mixed corpus')

// ---- the reference's error strings, and the window's range ----
assert.strictEqual(outcome(() => u.skipGramBatch(['ab', 'a☃'])), outcome(() => u.encodeToVectorBatch(['ab', 'a☃'])))
assert.strictEqual(outcome(() => u.skipGramBatch(['ab', 'a☃'])), 'error: unknown token, char: "☃"')
assert.strictEqual(outcome(() => u.skipGramBatchUtf8([Buffer.from('☃')])), 'error: unknown token, char: "☃"')
for (const w of [0, -1, 65, 1.5, '2']) {
  assert(/^error: skip-gram window/.test(outcome(() => u.skipGramBatch(mixed, w))), 'window ' + w)
  assert(/^error: skip-gram window/.test(outcome(() => u.skipGramBatchUtf8([Buffer.from('ab')], w))), 'window ' + w)
  assert(/^error: skip-gram window/.test(outcome(() => u.corpusToSkipGramBatch(null, w))), 'window ' + w)
}
assert(calls.skipGramTextBatch >= 8 && calls.skipGramUtf8Batch >= 9 && calls.exportSkipGram >= 6, JSON.stringify(calls))

console.log('skipgram_gpu ok: ' + JSON.stringify(calls))
