"""The skip-gram pair-count methods of the Node drop-in (bpe-tokenizer_amd/js/core.js over
addon/bpe_skipgram_counts_napi.node): the addon's exports, the methods and their typings on CPU; on
the GPU the three methods on golden cases and the error strings (tests/js/skipgram_counts_gpu.js)."""
import os
import shutil
import subprocess

import pytest

from bpe_amd import ROOT

NODE = shutil.which('node')
ADDON_DIR = os.path.join(ROOT, 'bpe-tokenizer_amd', 'addon')
CORE = os.path.join(ROOT, 'bpe-tokenizer_amd', 'js', 'core.js')
METHODS = ('skipGramCountsBatch', 'skipGramCountsBatchUtf8', 'corpusToSkipGramCounts')

pytestmark = pytest.mark.skipif(NODE is None, reason='node not installed')


def build_addon():
    subprocess.check_call(['make', '-s', '-C', ADDON_DIR])
    if not os.path.exists(os.path.join(ADDON_DIR, 'bpe_skipgram_counts_napi.node')):
        pytest.skip('no addon (node headers missing)')


def test_counts_addon_builds_and_exports():
    build_addon()
    out = subprocess.check_output([NODE, '-e', "const a=require(process.argv[1]);"
                                   "console.log(Object.keys(a).sort().join(','))",
                                   os.path.join(ADDON_DIR, 'bpe_skipgram_counts_napi.node')], text=True)
    assert out.strip() == 'exportSkipGramCounts,skipGramCountsTextBatch,skipGramCountsUtf8Batch'
    core = subprocess.check_output([NODE, '-e', "const {BPETokenizer}=require(process.argv[1]);"
                                    "console.log(process.argv.slice(2).map(k=>typeof BPETokenizer.prototype[k]).join(','))",
                                    CORE] + list(METHODS), text=True)
    assert core.strip() == 'function,function,function'
    dts = open(os.path.join(ROOT, 'bpe-tokenizer_amd', 'js', 'core.d.ts')).read()
    assert all('%s(' % m in dts for m in METHODS) and 'counts: Float64Array' in dts


@pytest.mark.gpu
def test_counts_methods_on_the_golden_cases_and_the_error_strings():
    """Every call through the device (BPE_ENCODE_DEVICE=1 lets its errors through)."""
    build_addon()
    out = subprocess.run([NODE, os.path.join(ROOT, 'tests', 'js', 'skipgram_counts_gpu.js')],
                         env=dict(os.environ, BPE_ENCODE_DEVICE='1'), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert 'skipgram_counts_gpu ok' in out.stdout
