// The corpus export of the Node drop-in (js/core.js and js/db.js over addon/bpe_export_napi.node,
// bpe_export_samples / bpe_export_text_batch on the GPU) on reference-generated golden cases
// (tests/golden/small_cases.json), after mergeUntil with the case's options:
//   corpus_in_code equals the reference's strings (final_ids: unit = index + 1);
//   corpusToVectorBatch() equals samples.map(encodeToVector), corpusToTextBatch() the samples,
//   both also for a list of indices with repeats;
//   the DB twin's rows after every applyMerge equal the reference's codes at that point (the
//   in-memory drop-in in lockstep), and a digest of all those rows is printed: the test compares it
//   between the device route and BPE_ENCODE_DEVICE=0, the route taken before.
// Run: node --expose-gc tests/js/spec_export_gpu.js
'use strict'
const assert = require('assert')
const crypto = require('crypto')
const fs = require('fs')
const os = require('os')
const path = require('path')
const { connectDB } = require('./sqlite_bridge')
const PKG = path.join(__dirname, '..', '..', 'bpe-tokenizer_amd', 'js')
const { BPETokenizer } = require(path.join(PKG, 'core.js'))
const { BPETokenizerDB, resetBPETokenizerDB } = require(path.join(PKG, 'db.js'))
const native = require(path.join(PKG, 'native.js'))

const JS_ROUTE = process.env.BPE_ENCODE_DEVICE === '0'

// whether the calls went through the addon
let calls = { exportSamples: 0, exportText: 0 }
if (!JS_ROUTE) {
  const addon = native.loadNativeExport()
  for (const name of Object.keys(calls)) {
    const inner = addon[name]
    addon[name] = function () {
      calls[name]++
      return inner.apply(this, arguments)
    }
  }
}

const cases = JSON.parse(fs.readFileSync(path.join(__dirname, '..', 'golden', 'small_cases.json'), 'utf8')).cases
const codeOf = ids => ids.map(i => String.fromCodePoint(i + 1)).join('')

let n_cases = 0
let n_vectors = 0
for (let k = 0; k < cases.length; k += 25) {
  const c = cases[k]
  if (global.gc) global.gc()
  const t = new BPETokenizer()
  for (const s of c.samples) t.addToCorpus(s)
  t.mergeUntil(c.opts)
  assert.deepStrictEqual(t.corpus_in_code, c.final_ids.map(codeOf), c.name)
  assert.deepStrictEqual(t.corpusToTextBatch(), c.samples, c.name)
  const n = c.samples.length
  const pick = n ? [n - 1, 0, n - 1] : []
  assert.deepStrictEqual(t.corpusToTextBatch(pick), pick.map(i => c.samples[i]), c.name)
  if (t.token_table.length) {
    const want = c.samples.map(s => t.encodeToVector(s))
    assert.deepStrictEqual(want, c.vectors, c.name)
    t.to_vector_index = null // (corpusToVectorBatch compacts the index itself, as encodeToVector does)
    const got = t.corpusToVectorBatch()
    assert.ok(got.every(v => v instanceof Int32Array), c.name)
    assert.deepStrictEqual(got.map(v => Array.from(v)), want, c.name)
    assert.deepStrictEqual(t.corpusToVectorBatch(pick).map(v => Array.from(v)), pick.map(i => want[i]), c.name)
    n_vectors += n
  }
  n_cases++
}
assert.ok(n_cases >= 60 && n_vectors > 150, [n_cases, n_vectors])

// a token the vector index skips: the reference's error string
{
  const t = new BPETokenizer()
  t.addToCorpus('abab')
  t.compactVectorIndex()
  delete t.to_vector_index[1]
  assert.throws(() => t.corpusToVectorBatch(), e => e.message === 'unknown token index: 1')
}

// the DB twin: rows after every applyMerge, in lockstep with the in-memory drop-in
const dir = fs.mkdtempSync(path.join(os.tmpdir(), 'bpe-export-gpu-'))
const db = connectDB(path.join(dir, 'BPE-tokenizer-test.sqlite3'))
const digest = crypto.createHash('sha256')
let n_rows = 0
for (let k = 3; k < cases.length; k += 150) {
  const c = cases[k]
  if (global.gc) global.gc()
  resetBPETokenizerDB(db)
  const tdb = new BPETokenizerDB({ db })
  const mem = new BPETokenizer()
  c.samples.forEach((s, i) => {
    tdb.addToCorpus(i + 1, s)
    mem.addToCorpus(s)
  })
  for (let it = 0; it < 12; it++) {
    const m = tdb.findNextMerge(c.opts)
    const mm = mem.findNextMerge(c.opts)
    assert.strictEqual(m === null, mm === null, c.name)
    if (!m) break
    tdb.applyMerge(m)
    mem.applyMerge(mm)
    const rows = Array.from(tdb.proxy.corpus).map(r => r.content_code)
    assert.deepStrictEqual(rows, mem.corpus_in_code, c.name)
    for (const r of rows) digest.update(r + '\n', 'utf8')
    n_rows += rows.length
  }
}
assert.ok(n_rows > 50, n_rows)

if (JS_ROUTE) assert.deepStrictEqual(calls, { exportSamples: 0, exportText: 0 })
else assert.ok(calls.exportSamples > n_cases && calls.exportText >= n_cases, JSON.stringify(calls))
console.log('route: ' + (JS_ROUTE ? 'js' : 'device'))
console.log('db rows digest: ' + digest.digest('hex') + ' ' + n_rows)
console.log('spec_export_gpu ok')
