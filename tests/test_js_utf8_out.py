"""The UTF-8 output methods of the Node drop-in (bpe-tokenizer_amd/js/core.js over
addon/bpe_utf8_out_napi.node): the addon's exports, the methods and their typings on CPU, the host
route without a device, and on the GPU the two methods against Buffer.from of the string methods
(tests/js/utf8_out_gpu.js)."""
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
    if not os.path.exists(os.path.join(ADDON_DIR, 'bpe_utf8_out_napi.node')):
        pytest.skip('no addon (node headers missing)')


def test_utf8_out_addon_builds_and_exports():
    build_addon()
    out = subprocess.check_output([NODE, '-e', "const a=require(process.argv[1]);"
                                   "console.log(Object.keys(a).sort().join(','))",
                                   os.path.join(ADDON_DIR, 'bpe_utf8_out_napi.node')], text=True)
    assert out.strip() == 'decodeUtf8Batch,exportUtf8'
    core = subprocess.check_output([NODE, '-e', "const {BPETokenizer}=require(process.argv[1]);"
                                    "console.log(['decodeVectorBatchUtf8','corpusToTextBatchUtf8']"
                                    ".map(k=>typeof BPETokenizer.prototype[k]).join(','))", CORE], text=True)
    assert core.strip() == 'function,function'
    dts = open(os.path.join(ROOT, 'bpe-tokenizer_amd', 'js', 'core.d.ts')).read()
    assert 'decodeVectorBatchUtf8(vectors: number[][]): Buffer[]' in dts
    assert 'corpusToTextBatchUtf8(indices?: number[]): Buffer[]' in dts


def test_without_a_device_the_decode_takes_the_string_route():
    if pkg.device_count() != 0:
        pytest.skip('a device is present: the GPU test covers the methods')
    build_addon()
    script = ("const {BPETokenizer}=require(process.argv[1]);const t=new BPETokenizer();"
              "t.fromJSON({version:2,char_count:3,token_table:[['a',1,1],['\\ud83d',1,1],['\\ude00',1,1]],merge_codes:[]});"
              "console.log(t.decodeVectorBatchUtf8([[0,1,2],[2,1],[]]).map(b=>b.toString('hex')).join(','));"
              "try{t.decodeVectorBatchUtf8([[7]])}catch(e){console.log(e.message)}")
    out = subprocess.run([NODE, '-e', script, CORE], capture_output=True, text=True)
    assert out.stdout.split() == ['61f09f9880,efbfbdefbfbd,', 'unknown', 'vector', 'index:', '7'], out.stdout + out.stderr


@pytest.mark.gpu
def test_utf8_out_methods_equal_buffer_from_of_the_string_methods():
    """decodeVectorBatchUtf8 and corpusToTextBatchUtf8 on a golden case and on texts with lone
    surrogates against Buffer.from of decodeVectorBatch / corpusToTextBatch, and the error string."""
    build_addon()
    out = subprocess.run([NODE, os.path.join(ROOT, 'tests', 'js', 'utf8_out_gpu.js')],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert 'utf8_out_gpu ok' in out.stdout
