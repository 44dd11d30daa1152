"""The skip-gram methods of the Node drop-in (bpe-tokenizer_amd/js/core.js over
addon/bpe_skipgram_napi.node): the addon's exports, the methods and their typings, and the JS route
against the reference's own pairs (tests/golden/skipgram_cases.json) on CPU; on the GPU the three
methods against the same class's encodeToVector per text, expanded by a per-token restatement in the
JS test (tests/js/skipgram_gpu.js)."""
import json
import os
import shutil
import subprocess

import pytest

from bpe_amd import ROOT

NODE = shutil.which('node')
ADDON_DIR = os.path.join(ROOT, 'bpe-tokenizer_amd', 'addon')
CORE = os.path.join(ROOT, 'bpe-tokenizer_amd', 'js', 'core.js')
NATIVE = os.path.join(ROOT, 'bpe-tokenizer_amd', 'js', 'native.js')

pytestmark = pytest.mark.skipif(NODE is None, reason='node not installed')


def build_addon():
    subprocess.check_call(['make', '-s', '-C', ADDON_DIR])
    if not os.path.exists(os.path.join(ADDON_DIR, 'bpe_skipgram_napi.node')):
        pytest.skip('no addon (node headers missing)')


def test_skipgram_addon_builds_and_exports():
    build_addon()
    out = subprocess.check_output([NODE, '-e', "const a=require(process.argv[1]);"
                                   "console.log(Object.keys(a).sort().join(','))",
                                   os.path.join(ADDON_DIR, 'bpe_skipgram_napi.node')], text=True)
    assert out.strip() == 'exportSkipGram,skipGramTextBatch,skipGramUtf8Batch'
    core = subprocess.check_output([NODE, '-e', "const {BPETokenizer}=require(process.argv[1]);"
                                    "console.log(['skipGramBatch','skipGramBatchUtf8','corpusToSkipGramBatch']"
                                    ".map(k=>typeof BPETokenizer.prototype[k]).join(','))", CORE], text=True)
    assert core.strip() == 'function,function,function'
    dts = open(os.path.join(ROOT, 'bpe-tokenizer_amd', 'js', 'core.d.ts')).read()
    assert 'skipGramBatch(texts: string[], window?: number): SkipGramPairs' in dts
    assert 'skipGramBatchUtf8(buffers: Array<Buffer | Uint8Array>, window?: number): SkipGramPairs' in dts
    assert 'corpusToSkipGramBatch(indices?: number[] | null, window?: number): SkipGramPairs' in dts


def test_the_js_route_equals_every_golden_case():
    """expandSkipGram (js/native.js), what a call the device cannot take runs, on the fixture's arrays:
    each case alone and each window's cases as one batch; the window's default and its range."""
    with open(os.path.join(ROOT, 'tests', 'golden', 'skipgram_cases.json')) as f:
        cases = json.load(f)['cases']
    script = ("const n=require(process.argv[1]);const cases=JSON.parse(require('fs').readFileSync(process.argv[2])).cases;"
              "const out=cases.map(c=>{const r=n.expandSkipGram([c.values],c.window);"
              "return [Array.from(r.targets),Array.from(r.contexts),Array.from(r.offsets)]});"
              "const all=[1,2,3,5].map(w=>{const r=n.expandSkipGram(cases.filter(c=>c.window===w).map(c=>c.values),w);"
              "return [Array.from(r.targets),Array.from(r.contexts),Array.from(r.offsets)]});"
              "const bad=[0,-1,65,1.5].map(w=>{try{n.skipGramWindow(w);return 'ok'}catch(e){return e.message}});"
              "console.log(JSON.stringify({out,all,bad,dflt:n.skipGramWindow(undefined),top:n.skipGramWindow(64)}))")
    res = json.loads(subprocess.check_output(
        [NODE, '-e', script, NATIVE, os.path.join(ROOT, 'tests', 'golden', 'skipgram_cases.json')], text=True))
    for c, (t, x, off) in zip(cases, res['out']):
        assert [list(p) for p in zip(t, x)] == c['pairs'] and off == [0, len(c['pairs'])], (c['window'], len(c['values']))
    for w, (t, x, off) in zip((1, 2, 3, 5), res['all']):
        mine = [c for c in cases if c['window'] == w]
        assert [list(p) for p in zip(t, x)] == [p for c in mine for p in c['pairs']]
        assert off == [0] + [sum(len(c['pairs']) for c in mine[:k + 1]) for k in range(len(mine))]
    assert all(b.startswith('skip-gram window') for b in res['bad']) and res['dflt'] == 2 and res['top'] == 64


@pytest.mark.gpu
def test_skipgram_methods_equal_the_rule_on_encode_to_vector():
    """skipGramBatch, skipGramBatchUtf8 and corpusToSkipGramBatch on a golden case and on texts of
    several scripts, every call through the device (BPE_ENCODE_DEVICE=1 lets its errors through), the
    default window, and the error strings."""
    build_addon()
    out = subprocess.run([NODE, os.path.join(ROOT, 'tests', 'js', 'skipgram_gpu.js')],
                         env=dict(os.environ, BPE_ENCODE_DEVICE='1'), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert 'skipgram_gpu ok' in out.stdout
