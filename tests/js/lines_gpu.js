// BPETokenizer.addLinesToCorpusBatch / addLinesToCorpusBatchUtf8 / restoreLinesToCorpusBatch /
// restoreLinesToCorpusBatchUtf8 (js/core.js over addon/bpe_lines_napi.node: the texts are split into
// samples on the GPU) against the same class fed `texts.flatMap(helper)` through the existing string
// methods: toJSON(), corpus_in_code and the merges that follow are equal, for each of the three
// helpers.  Files: the first 256 KiB of the golden config's stream (tests/golden/config2.json: seed,
// alphabet) with a line end planted every few dozen bytes, texts of several scripts with every kind
// of whitespace at the line ends, ill-formed bytes, an empty file.  An unknown char throws the
// reference's string and an unknown helper throws.
// Run: node tests/js/lines_gpu.js
'use strict'
const assert = require('assert')
const path = require('path')
const fs = require('fs')
const core = require(path.join(__dirname, '..', '..', 'bpe-tokenizer_amd', 'js', 'core.js'))
const native = require(path.join(__dirname, '..', '..', 'bpe-tokenizer_amd', 'js', 'native.js'))
const { BPETokenizer } = core

const g = JSON.parse(fs.readFileSync(path.join(__dirname, '..', 'golden', 'config2.json')))

// whether the batches went through the native calls
const calls = { addLinesBatch: 0, addLinesUtf8Batch: 0, restoreLinesBatch: 0, restoreLinesUtf8Batch: 0 }
const addon = native.loadNativeLines()
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

const stream = xorshiftBytes(g.seed, g.A, g.base, 1 << 18)
const ends = [[0x0a], [0x0d, 0x0a], [0x20, 0x0a, 0x09], [0x0d], [0x0a, 0x0a]]
for (let i = 17, k = 0; i + 3 < stream.length; i += 23 + (k % 31), k++) Buffer.from(ends[k % ends.length]).copy(stream, i)
const buffers = []
for (let off = 0; off < stream.length; off += 1 << 16) buffers.push(stream.slice(off, off + (1 << 16)))
buffers.push(Buffer.from('  Съешь ещё\u3000\r\n\tэтих мягких булок \n\n色は匂へど 😀🎉 \n\ufeff naïve \x1c\x85\u200b \r'))
buffers.push(Buffer.alloc(0))
buffers.push(Buffer.from([0x20, 0x61, 0xff, 0x0a, 0xe2, 0x82, 0x20, 0x0a, 0xf0, 0x9f, 0x98]))   // ill-formed: three U+FFFD
buffers.push(new Uint8Array([0x0a, 0xc0, 0xaf, 0x0d, 0x0a, 0x7a]))
const str = b => Buffer.from(b.buffer, b.byteOffset, b.length).toString()
const texts = buffers.map(str)

const HELPERS = {
  linesToCorpus: core.linesToCorpus,
  linesTrimmedToCorpus: core.linesTrimmedToCorpus,
  fileContentToCorpus: t => [core.fileContentToCorpus(t)],
}
function flatMap(list, helper) {
  const out = []
  for (const t of list) for (const s of HELPERS[helper](t)) out.push(s)
  return out
}

function mergesOf(t) {
  return t.merge_tokens.map(([x, y, z]) => [x.index, y.index, z.index])
}

function same(a, b, what) {
  assert.deepStrictEqual(a.corpus_in_code, b.corpus_in_code, what + ': corpus_in_code')
  assert.deepStrictEqual(JSON.parse(JSON.stringify(a.toJSON())), JSON.parse(JSON.stringify(b.toJSON())), what + ': toJSON')
}

function outcome(fn) {
  try {
    return fn()
  } catch (e) {
    return 'error: ' + e.message
  }
}

for (const helper of Object.keys(HELPERS)) {
  const arg = helper === 'linesToCorpus' ? undefined : helper   // (the default)
  // ---- ingest from strings and from bytes, in two calls each, then training ----
  const want = new BPETokenizer()
  for (const s of flatMap(texts, helper)) want.addToCorpus(s)
  const a = new BPETokenizer()
  const b = new BPETokenizer()
  a.addLinesToCorpusBatch(texts.slice(0, 3), arg)
  a.addLinesToCorpusBatch(texts.slice(3), arg)
  a.addLinesToCorpusBatch([], arg)
  b.addLinesToCorpusBatchUtf8(buffers.slice(0, 3), arg)
  b.addLinesToCorpusBatchUtf8(buffers.slice(3), arg)
  same(a, want, helper + ': ingest from strings')
  same(b, want, helper + ': ingest from bytes')
  assert.deepStrictEqual(Object.keys(a.char_to_token), Object.keys(want.char_to_token))
  assert.deepStrictEqual(Object.keys(b.char_to_token), Object.keys(want.char_to_token))
  assert.strictEqual(a.token_table[0].chars, helper === 'fileContentToCorpus' ? '\x1c' : '\r')
  assert('\ufffd' in b.char_to_token)
  for (const t of [a, b, want]) t.mergeUntil({ min_weight: 2, max_iterations: 30 })
  assert.deepStrictEqual(mergesOf(a), mergesOf(want), helper + ': merges')
  assert.deepStrictEqual(mergesOf(b), mergesOf(want), helper + ': merges from bytes')
  same(a, want, helper + ': after 30 merges')
  same(b, want, helper + ': after 30 merges, from bytes')

  // ---- restore into tokenizers made by fromJSON ----
  const json = JSON.parse(JSON.stringify(a.toJSON()))
  const ra = new BPETokenizer()
  const rb = new BPETokenizer()
  const rw = new BPETokenizer()
  for (const t of [ra, rb, rw]) t.fromJSON(json)
  ra.restoreLinesToCorpusBatch(texts, arg)
  rb.restoreLinesToCorpusBatchUtf8(buffers, arg)
  for (const s of flatMap(texts, helper)) rw.restoreToCorpus(s)
  same(ra, rw, helper + ': restore')
  same(rb, rw, helper + ': restore from bytes')
  assert.deepStrictEqual(ra.corpus_in_code, a.corpus_in_code, helper + ': the trained corpus')
  for (const t of [ra, rb, rw]) t.mergeUntil({ min_weight: 2, max_iterations: 10 })
  assert.deepStrictEqual(mergesOf(ra), mergesOf(rw), helper + ': merges after the restore')
  assert.deepStrictEqual(mergesOf(rb), mergesOf(rw), helper + ': merges after the restore from bytes')
  same(ra, rw, helper + ': restore, then 10 merges')

  // ---- an unknown char: the reference's string, and nothing added ----
  const fresh = new BPETokenizer()
  fresh.fromJSON(json)
  const n_before = fresh.corpus_in_code.length
  assert.strictEqual(outcome(() => fresh.restoreLinesToCorpusBatch(['a\n', ' a☃ \nz'], arg)), 'error: unknown token, char: "☃"')
  assert.strictEqual(outcome(() => fresh.restoreLinesToCorpusBatchUtf8([Buffer.from('a\n ☃')], arg)),
    'error: unknown token, char: "☃"')
  assert.strictEqual(fresh.corpus_in_code.length, n_before)
}

// ---- an unknown helper throws, whatever else is wrong ----
const t = new BPETokenizer()
for (const m of ['addLinesToCorpusBatch', 'addLinesToCorpusBatchUtf8', 'restoreLinesToCorpusBatch', 'restoreLinesToCorpusBatchUtf8']) {
  assert(/^error: unknown corpus helper: trim /.test(outcome(() => t[m]([], 'trim'))), m)
}
assert.strictEqual(calls.addLinesBatch, 6)
assert.strictEqual(calls.addLinesUtf8Batch, 6)
assert(calls.restoreLinesBatch >= 6 && calls.restoreLinesUtf8Batch >= 6, JSON.stringify(calls))

console.log('lines_gpu ok: ' + buffers.length + ' files, ' + JSON.stringify(calls))
