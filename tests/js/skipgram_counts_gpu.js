// BPETokenizer.skipGramCountsBatch / skipGramCountsBatchUtf8 / corpusToSkipGramCounts (js/core.js over
// addon/bpe_skipgram_counts_napi.node: encoded or exported, and counted, on the GPU) against the
// reference's own pairs (tests/golden/skipgram_cases.json) counted here, and against the same class's
// encodeToVector per text under the rule restated below, on a golden case (tests/golden/small_cases.json).
// Run: node tests/js/skipgram_counts_gpu.js
'use strict'
const assert = require('assert')
const path = require('path')
const fs = require('fs')
const { BPETokenizer } = require(path.join(__dirname, '..', '..', 'bpe-tokenizer_amd', 'js', 'core.js'))
const native = require(path.join(__dirname, '..', '..', 'bpe-tokenizer_amd', 'js', 'native.js'))

// whether the batches went through the native calls
const calls = { skipGramCountsTextBatch: 0, skipGramCountsUtf8Batch: 0, exportSkipGramCounts: 0 }
const addon = native.loadNativeSkipGramCounts()
for (const name of Object.keys(calls)) {
  const inner = addon[name]
  addon[name] = function () {
    calls[name]++
    return inner.apply(this, arguments)
  }
}

// pairs [[target, context], ...] -> 'target,context' -> count, as sorted rows [target, context, count]
function counted(pairs) {
  const cells = new Map()
  for (const [t, c] of pairs) cells.set(t + ',' + c, (cells.get(t + ',' + c) || 0) + 1)
  return Array.from(cells, ([k, n]) => k.split(',').map(Number).concat(n)).sort((a, b) => a[0] - b[0] || a[1] - b[1])
}

// the rule: token i's contexts are the places i - w .. i + w without i and the places outside the text
function rule(vectors, w) {
  const pairs = []
  for (const v of vectors)
    for (let i = 0; i < v.length; i++)
      for (let d = -w; d <= w; d++) if (d !== 0 && i + d >= 0 && i + d < v.length) pairs.push([v[i], v[i + d]])
  return pairs
}

function same(got, pairs, what) {
  assert(got.targets instanceof Int32Array && got.contexts instanceof Int32Array && got.counts instanceof Float64Array, what)
  assert.deepStrictEqual(Array.from(got.targets, (t, u) => [t, got.contexts[u], got.counts[u]]), counted(pairs), what)
}

function outcome(fn) {
  try {
    return fn()
  } catch (e) {
    return 'error: ' + e.message
  }
}

// ---- the JS route on the reference's own pairs, each window's cases as one batch ----
const golden = JSON.parse(fs.readFileSync(path.join(__dirname, '..', 'golden', 'skipgram_cases.json'))).cases
for (const w of [1, 2, 3, 5]) {
  const mine = golden.filter(c => c.window === w)
  same(native.countSkipGram(mine.map(c => c.values), w, 65536), [].concat(...mine.map(c => c.pairs)), 'JS route, window ' + w)
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
for (const w of [1, 2, 5, 64]) {
  same(t.skipGramCountsBatch(texts, w), rule(vectors, w), 'texts, window ' + w)
  same(t.skipGramCountsBatchUtf8(texts.map(s => Buffer.from(s)), w), rule(vectors, w), 'buffers, window ' + w)
  same(t.corpusToSkipGramCounts(null, w), rule(g.vectors, w), 'corpus, window ' + w)
}
same(t.skipGramCountsBatch(texts), rule(vectors, 2), 'texts, default window')
same(t.corpusToSkipGramCounts([2, 0, 0]), rule([2, 0, 0].map(k => g.vectors[k]), 2), 'chosen samples')
same(t.corpusToSkipGramCounts([]), [], 'no sample')
same(t.skipGramCountsBatch([]), [], 'no text')
same(new BPETokenizer().corpusToSkipGramCounts(), [], 'no corpus')
assert(t.skipGramCountsBatch(texts).targets.length > 50)

// ---- the reference's error strings, and the window's range ----
const bad = ['☃', '§', '¤'].find(ch => !g.samples.some(s => s.includes(ch)))
assert.strictEqual(outcome(() => t.skipGramCountsBatch([bad])), outcome(() => t.encodeToVectorBatch([bad])))
assert.strictEqual(outcome(() => t.skipGramCountsBatch([bad])), 'error: unknown token, char: ' + JSON.stringify(bad))
assert.strictEqual(outcome(() => t.skipGramCountsBatchUtf8([Buffer.from(bad)])), 'error: unknown token, char: ' + JSON.stringify(bad))
for (const w of [0, 65, 1.5]) {
  assert(/^error: skip-gram window/.test(outcome(() => t.skipGramCountsBatch(texts, w))), 'window ' + w)
  assert(/^error: skip-gram window/.test(outcome(() => t.skipGramCountsBatchUtf8([Buffer.from('ab')], w))), 'window ' + w)
  assert(/^error: skip-gram window/.test(outcome(() => t.corpusToSkipGramCounts(null, w))), 'window ' + w)
}
assert(calls.skipGramCountsTextBatch >= 6 && calls.skipGramCountsUtf8Batch >= 5 && calls.exportSkipGramCounts >= 6, JSON.stringify(calls))

console.log('skipgram_counts_gpu ok: ' + JSON.stringify(calls))
