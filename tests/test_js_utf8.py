"""The UTF-8 batch methods of the Node drop-in (bpe-tokenizer_amd/js/core.js over
addon/bpe_utf8_napi.node): the addon's exports and the methods on CPU, and on the GPU the three
methods on Buffers against the same class fed `b.toString()` through the existing batch methods
(tests/js/utf8_gpu.js)."""
import os
import shutil
import subprocess

import pytest

from bpe_amd import ROOT, pkg

NODE = shutil.which('node')
ADDON_DIR = os.path.join(ROOT, 'bpe-tokenizer_amd', 'addon')
CORE = os.path.join(ROOT, 'bpe-tokenizer_amd', 'js', 'core.js')

pytestmark = pytest.mark.skipif(NODE is None, reason='node not installed')


def build_addon():
    subprocess.check_call(['make', '-s', '-C', ADDON_DIR])
    if not os.path.exists(os.path.join(ADDON_DIR, 'bpe_utf8_napi.node')):
        pytest.skip('no addon (node headers missing)')


def test_utf8_addon_builds_and_exports():
    build_addon()
    out = subprocess.check_output([NODE, '-e', "const a=require(process.argv[1]);"
                                   "console.log(Object.keys(a).sort().join(','))",
                                   os.path.join(ADDON_DIR, 'bpe_utf8_napi.node')], text=True)
    assert out.strip() == 'addUtf8Batch,encodeUtf8Batch,restoreUtf8Batch'
    core = subprocess.check_output([NODE, '-e', "const {BPETokenizer}=require(process.argv[1]);"
                                    "console.log(['addToCorpusBatchUtf8','restoreToCorpusBatchUtf8',"
                                    "'encodeToVectorBatchUtf8'].map(k=>typeof BPETokenizer.prototype[k]).join(','))",
                                    CORE], text=True)
    assert core.strip() == 'function,function,function'
    dts = open(os.path.join(ROOT, 'bpe-tokenizer_amd', 'js', 'core.d.ts')).read()
    for name in ('addToCorpusBatchUtf8', 'restoreToCorpusBatchUtf8', 'encodeToVectorBatchUtf8'):
        assert name + '(buffers: Array<Buffer | Uint8Array>)' in dts


def test_without_a_device_the_ingest_fails_with_the_usual_error():
    if pkg.device_count() != 0:
        pytest.skip('a device is present: the GPU test covers the methods')
    build_addon()
    out = subprocess.run([NODE, '-e', "const {BPETokenizer}=require(process.argv[1]);const t=new BPETokenizer();"
                          "try{t.addToCorpusBatchUtf8([Buffer.from('ab')]);console.log('no error')}"
                          "catch(e){console.log(e.message)}", CORE], capture_output=True, text=True)
    assert 'no HIP device' in out.stdout, out.stdout + out.stderr


@pytest.mark.gpu
def test_utf8_batch_methods_equal_the_string_methods_on_to_string():
    """addToCorpusBatchUtf8, encodeToVectorBatchUtf8 and restoreToCorpusBatchUtf8 on Buffers (the golden
    config's stream, several scripts, ill-formed bytes, empty buffers) against the string methods on
    b.toString(): toJSON(), corpus_in_code, merges, vectors, and one unknown-char error string."""
    build_addon()
    out = subprocess.run([NODE, os.path.join(ROOT, 'tests', 'js', 'utf8_gpu.js')],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert 'utf8_gpu ok' in out.stdout
