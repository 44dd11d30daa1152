"""BPETokenizer.encodeToVectorBatch of the Node drop-in (bpe-tokenizer_amd/js/core.js over
addon/bpe_text_napi.node): the text encoder's addon and the JS fallback on CPU
(tests/js/text_encoder_host.js), the batch encode against the reference's own encodeToVector loop
on the GPU (tests/js/text_encoder_gpu.js)."""
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
    if not os.path.exists(os.path.join(ADDON_DIR, 'bpe_text_napi.node')):
        pytest.skip('no addon (node headers missing)')


def test_text_addon_builds_and_exports():
    build_addon()
    out = subprocess.check_output([NODE, '-e', "const a=require(process.argv[1]);"
                                   "console.log(Object.keys(a).sort().join(','))",
                                   os.path.join(ADDON_DIR, 'bpe_text_napi.node')], text=True)
    assert out.strip() == ('createTextEncoder,destroyTextEncoder,encodeTextBatch,textEncoderAddMerges,'
                           'textEncoderClear,textEncoderSetChars,textEncoderSetVectorIndex')


def test_batch_equals_mapped_encode_to_vector_without_forcing_the_device():
    """BPE_ENCODE_DEVICE unset: without a device the JS fallback takes over; 50 small golden cases,
    both error strings, an empty batch, an empty table."""
    build_addon()
    env = {k: v for k, v in os.environ.items() if k != 'BPE_ENCODE_DEVICE'}
    out = subprocess.run([NODE, os.path.join(ROOT, 'tests', 'js', 'text_encoder_host.js')], env=env,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert 'text_encoder_host ok' in out.stdout


@pytest.mark.gpu
def test_encode_to_vector_batch_equals_mapped_encode_to_vector():
    """encodeToVectorBatch == texts.map(encodeToVector) on the config 2 golden and 50 small cases,
    the encoder following fromJSON, applyMerge and addToCorpus, both error strings, and the round
    trip through decodeVectorBatch."""
    build_addon()
    out = subprocess.run([NODE, os.path.join(ROOT, 'tests', 'js', 'text_encoder_gpu.js')],
                         env=dict(os.environ, BPE_ENCODE_DEVICE='1'),
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert 'text_encoder_gpu ok' in out.stdout
