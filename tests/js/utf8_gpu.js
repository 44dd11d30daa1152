// BPETokenizer.addToCorpusBatchUtf8 / restoreToCorpusBatchUtf8 / encodeToVectorBatchUtf8 (js/core.js over
// addon/bpe_utf8_napi.node: the UTF-8 bytes are decoded on the GPU) against the same class fed
// `b.toString()` through the existing batch methods: toJSON(), corpus_in_code, the merges that follow
// and the vectors are equal.  Buffers: the first MiB of the golden config's stream (tests/golden/
// config2.json: seed, alphabet) in 64 KiB samples, texts of several scripts, ill-formed bytes, empty
// buffers and a Uint8Array.  An unknown char throws the reference's string.
// Run: node tests/js/utf8_gpu.js
'use strict'
const assert = require('assert')
const path = require('path')
const fs = require('fs')
const { BPETokenizer } = require(path.join(__dirname, '..', '..', 'bpe-tokenizer_amd', 'js', 'core.js'))
const native = require(path.join(__dirname, '..', '..', 'bpe-tokenizer_amd', 'js', 'native.js'))

const g = JSON.parse(fs.readFileSync(path.join(__dirname, '..', 'golden', 'config2.json')))

// whether the batches went through the native calls
const calls = { addUtf8Batch: 0, restoreUtf8Batch: 0, encodeUtf8Batch: 0 }
const addon = native.loadNativeUtf8()
for (const name of Object.keys(calls)) {
  const inner = addon[name]
  addon[name] = function () {
    calls[name]++
    return inner.apply(this, arguments)
  }
}

function xorshiftBytes(seed, A, base, n) {
  const out = Buffer.alloc(n)
  let x = seed >>> 0
  for (let i = 0; i < n; i++) {
    x ^= x << 13; x >>>= 0
    x ^= x >>> 17
    x ^= x << 5; x >>>= 0
    out[i] = base + Math.floor(x * A / 4294967296)
  }
  return out
}

const stream = xorshiftBytes(g.seed, g.A, g.base, 1 << 20)
const buffers = []
for (let off = 0; off < stream.length; off += 1 << 16) buffers.push(stream.slice(off, off + (1 << 16)))
buffers.push(Buffer.from('Съешь ещё этих мягких булок 色は匂へど 😀🎉 naïve \ufeff\ufffd'))
buffers.push(Buffer.alloc(0))
buffers.push(Buffer.from([0x61, 0xff, 0x62, 0xe2, 0x82, 0x63, 0xf0, 0x9f, 0x98]))   // ill-formed: three U+FFFD
buffers.push(new Uint8Array([0xc0, 0xaf, 0xed, 0xa0, 0x80, 0x7a]))
const str = b => Buffer.from(b.buffer, b.byteOffset, b.length).toString()
const texts = buffers.map(str)
assert(texts[texts.length - 2].includes('\ufffd'))

function mergesOf(t) {
  return t.merge_tokens.map(([x, y, z]) => [x.index, y.index, z.index])
}

function same(a, b, what) {
  assert.deepStrictEqual(a.corpus_in_code, b.corpus_in_code, what + ': corpus_in_code')
  assert.deepStrictEqual(JSON.parse(JSON.stringify(a.toJSON())), JSON.parse(JSON.stringify(b.toJSON())), what + ': toJSON')
}

// ---- ingest, in two calls (the second meets a filled char table), then training ----
const a = new BPETokenizer()
const b = new BPETokenizer()
a.addToCorpusBatchUtf8(buffers.slice(0, 10))
a.addToCorpusBatchUtf8(buffers.slice(10))
a.addToCorpusBatchUtf8([])
b.addToCorpusBatch(texts.slice(0, 10))
b.addToCorpusBatch(texts.slice(10))
assert.strictEqual(calls.addUtf8Batch, 2)
same(a, b, 'ingest')
assert.deepStrictEqual(Object.keys(a.char_to_token), Object.keys(b.char_to_token))
assert('\ufffd' in a.char_to_token)
a.mergeUntil({ min_weight: 2, max_iterations: 30 })
b.mergeUntil({ min_weight: 2, max_iterations: 30 })
assert.deepStrictEqual(mergesOf(a), mergesOf(b), 'merges')
same(a, b, 'after 30 merges')

// ---- vectors ----
const va = a.encodeToVectorBatchUtf8(buffers)
const vb = b.encodeToVectorBatch(texts)
assert.deepStrictEqual(va, vb, 'vectors')
assert.deepStrictEqual(va[va.length - 1], b.encodeToVector(texts[texts.length - 1]))
assert.deepStrictEqual(a.encodeToVectorBatchUtf8([]), [])

// ---- restore into tokenizers made by fromJSON ----
const json = JSON.parse(JSON.stringify(a.toJSON()))
const ra = new BPETokenizer()
const rb = new BPETokenizer()
ra.fromJSON(json)
rb.fromJSON(json)
ra.restoreToCorpusBatchUtf8(buffers)
rb.restoreToCorpusBatch(texts)
same(ra, rb, 'restore')
assert.deepStrictEqual(ra.corpus_in_code, a.corpus_in_code, 'the trained corpus')
ra.mergeUntil({ min_weight: 2, max_iterations: 10 })
rb.mergeUntil({ min_weight: 2, max_iterations: 10 })
assert.deepStrictEqual(mergesOf(ra), mergesOf(rb), 'merges after the restore')
same(ra, rb, 'restore, then 10 merges')

// ---- an unknown char: the reference's string, from all three routes alike ----
function outcome(fn) {
  try {
    return fn()
  } catch (e) {
    return 'error: ' + e.message
  }
}
const fresh = new BPETokenizer()
fresh.fromJSON(json)
const bad = [Buffer.from('abc'), Buffer.from([0x61, 0xe2, 0x98, 0x83])]   // U+2603 is in no table
const n_before = fresh.corpus_in_code.length
assert.strictEqual(outcome(() => fresh.encodeToVectorBatchUtf8(bad)), 'error: unknown token, char: "☃"')
assert.strictEqual(outcome(() => fresh.encodeToVectorBatchUtf8(bad)), outcome(() => fresh.encodeToVectorBatch(bad.map(str))))
assert.strictEqual(outcome(() => fresh.restoreToCorpusBatchUtf8(bad)), 'error: unknown token, char: "☃"')
assert.strictEqual(fresh.corpus_in_code.length, n_before)
assert(calls.encodeUtf8Batch >= 2 && calls.restoreUtf8Batch >= 2, JSON.stringify(calls))

console.log('utf8_gpu ok: ' + buffers.length + ' buffers, ' + JSON.stringify(calls))
