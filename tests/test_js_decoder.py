"""BPETokenizer.decodeVectorBatch of the Node drop-in (bpe-tokenizer_amd/js/core.js over
addon/bpe_decode_napi.node): the decoder's addon on CPU, the batch decode against the reference's
own decodeVector loop on the GPU (tests/js/decoder_gpu.js)."""
import os
import shutil
import subprocess

import pytest

from bpe_amd import ROOT

NODE = shutil.which('node')
ADDON_DIR = os.path.join(ROOT, 'bpe-tokenizer_amd', 'addon')

pytestmark = pytest.mark.skipif(NODE is None, reason='node not installed')


def build_addon():
    subprocess.check_call(['make', '-s', '-C', ADDON_DIR])
    if not os.path.exists(os.path.join(ADDON_DIR, 'bpe_decode_napi.node')):
        pytest.skip('no addon (node headers missing)')


def test_decoder_addon_builds_and_exports():
    build_addon()
    out = subprocess.check_output([NODE, '-e', "const a=require(process.argv[1]);"
                                   "console.log(Object.keys(a).sort().join(','))",
                                   os.path.join(ADDON_DIR, 'bpe_decode_napi.node')], text=True)
    assert out.strip() == ('createDecoder,decodeBatch,decoderAddMerges,decoderAddTokens,decoderClear,'
                           'decoderSetVectorIndex,destroyDecoder')


@pytest.mark.gpu
def test_decode_vector_batch_equals_mapped_decode_vector():
    """decodeVectorBatch == vectors.map(decodeVector) on the config 2 golden and 50 small cases,
    the reference's error string for an unknown index, the decoder rebuilt after fromJSON."""
    build_addon()
    out = subprocess.run([NODE, os.path.join(ROOT, 'tests', 'js', 'decoder_gpu.js')],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert 'decoder_gpu ok' in out.stdout
