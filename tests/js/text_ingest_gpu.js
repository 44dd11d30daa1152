// BPETokenizer.addToCorpusBatch (js/core.js over addon/bpe_ingest_napi.node, bpe_add_text_batch on the
// GPU) against the reference's own loop, addToCorpus (core.ts:182-207), on a second instance: toJSON()
// deep-equal, corpus_in_code equal, mergeUntil equal, encodeToVector equal; on golden cases, on texts
// with lone surrogates and empty texts, after host-side addToCorpus calls, after merges, and after
// fromJSON on a fresh instance.
// Run: node tests/js/text_ingest_gpu.js
'use strict'
const assert = require('assert')
const path = require('path')
const fs = require('fs')
const { BPETokenizer } = require(path.join(__dirname, '..', '..', 'bpe-tokenizer_amd', 'js', 'core.js'))

// a call's value, or the message of what it throws (an empty token table throws in both)
function outcome(fn) {
  try {
    return fn()
  } catch (e) {
    return 'error: ' + e.message
  }
}

function same(a, b, texts, what) {
  assert.deepStrictEqual(a.toJSON(), b.toJSON(), what + ': toJSON')
  assert.deepStrictEqual(Object.keys(a.char_to_token), Object.keys(b.char_to_token), what + ': char_to_token')
  assert.deepStrictEqual(Object.keys(a.code_to_token), Object.keys(b.code_to_token), what + ': code_to_token')
  assert.deepStrictEqual(a.token_table, b.token_table, what + ': token_table')
  assert.deepStrictEqual(a.corpus_in_code, b.corpus_in_code, what + ': corpus_in_code')
  for (const t of texts)
    assert.deepStrictEqual(outcome(() => a.encodeToVector(t)), outcome(() => b.encodeToVector(t)), what + ': encodeToVector')
}

function both(texts, opts, what) {
  const a = new BPETokenizer()
  const b = new BPETokenizer()
  a.addToCorpusBatch(texts)
  for (const t of texts) b.addToCorpus(t)
  same(a, b, texts, what)
  a.mergeUntil(opts)
  b.mergeUntil(opts)
  same(a, b, texts, what + ' after mergeUntil')
  return [a, b]
}

// ---- golden cases: every case beyond latin1 among the first 400, and every 10th of the others ----
const cases = JSON.parse(fs.readFileSync(path.join(__dirname, '..', 'golden', 'small_cases.json'))).cases
let n_cases = 0
cases.slice(0, 400).forEach((c, i) => {
  const wide = c.samples.some(s => /[^\u0000-ÿ]/.test(s))
  if (!wide && i % 10) return
  const [a] = both(c.samples, c.opts, c.name)
  assert.deepStrictEqual(a.merge_tokens.map(([x, y, z]) => [x.index, y.index, z.original_weight]), c.merges, c.name)
  n_cases++
})
assert.ok(n_cases >= 60, String(n_cases))

// ---- lone surrogates, a text boundary inside a pair, empty texts ------------------------------
const G = '\u{1F600}'
const texts = ['', 'ab' + '\ud83d', '\ude00' + 'c' + G, '', '', 'x'.repeat(3000) + G + '中Ж', '\udc00\ud800', '']
const [a, b] = both(texts, { min_weight: 2, max_length: 3, max_iterations: 20 }, 'surrogates')

// ---- after merges: new chars are numbered past the merged tokens --------------------------------
const more = ['abнов' + G, '', 'q\u{20000}q\u{20000}', 'abab']
a.addToCorpusBatch(more)
for (const t of more) b.addToCorpus(t)
same(a, b, texts.concat(more), 'a batch after merges')
a.mergeUntil({ max_iterations: 10 })
b.mergeUntil({ max_iterations: 10 })
same(a, b, texts.concat(more), 'training after the second batch')

// ---- chars added on the host in between: the engine's table follows char_to_token -------------
const c1 = new BPETokenizer()
const c2 = new BPETokenizer()
c1.addToCorpus('hello')
c1.addToCorpusBatch(['world', 'hello' + G])
c1.addToCorpus('zebra' + G + '中')
c1.addToCorpusBatch(['中z', 'new!'])
for (const t of ['hello', 'world', 'hello' + G, 'zebra' + G + '中', '中z', 'new!']) c2.addToCorpus(t)
same(c1, c2, ['hello', 'new!'], 'mixed with addToCorpus')

// ---- after fromJSON on a fresh instance ------------------------------------------------------------
const json = JSON.parse(JSON.stringify(b.toJSON()))
const d1 = new BPETokenizer()
const d2 = new BPETokenizer()
d1.fromJSON(json)
d2.fromJSON(json)
const again = ['abab' + G, 'ωab', '', 'q\u{20000}ω']
d1.addToCorpusBatch(again)
for (const t of again) d2.addToCorpus(t)
same(d1, d2, again, 'after fromJSON')
d1.mergeUntil({ max_iterations: 5 })
d2.mergeUntil({ max_iterations: 5 })
same(d1, d2, again, 'training after fromJSON')

// ---- an empty batch changes nothing ------------------------------------------------------------------
const before = JSON.stringify(d1.toJSON())
d1.addToCorpusBatch([])
assert.strictEqual(JSON.stringify(d1.toJSON()), before)

console.log('text_ingest_gpu ok: ' + n_cases + ' golden cases')
