"""BPETokenizer.restoreToCorpusBatch of the Node drop-in (bpe-tokenizer_amd/js/core.js over
addon/bpe_restore_napi.node): the addon's exports on CPU, and the batch restore against the reference's
own restoreToCorpus loop on the GPU (tests/js/spec_restore_gpu.js)."""
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
    if not os.path.exists(os.path.join(ADDON_DIR, 'bpe_restore_napi.node')):
        pytest.skip('no addon (node headers missing)')


def test_restore_addon_builds_and_exports():
    build_addon()
    out = subprocess.check_output([NODE, '-e', "const a=require(process.argv[1]);"
                                   "console.log(Object.keys(a).sort().join(','))",
                                   os.path.join(ADDON_DIR, 'bpe_restore_napi.node')], text=True)
    assert out.strip() == 'addSampleBatch,restoreTextBatch'
    core = subprocess.check_output([NODE, '-e', "const {BPETokenizer}=require(process.argv[1]);"
                                    "console.log(typeof BPETokenizer.prototype.restoreToCorpusBatch)",
                                    os.path.join(ROOT, 'bpe-tokenizer_amd', 'js', 'core.js')], text=True)
    assert core.strip() == 'function'


def run_spec(env=None):
    build_addon()
    out = subprocess.run([NODE, os.path.join(ROOT, 'tests', 'js', 'spec_restore_gpu.js')],
                         capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return out.stdout


@pytest.mark.gpu
def test_restore_to_corpus_batch_equals_a_loop_of_restore_to_corpus():
    """restoreToCorpusBatch(contents) on a tokenizer restored by fromJSON from golden cases against a
    loop of restoreToCorpus on a second instance: corpus_in_code, toJSON() and the next 20 merges
    agree; an unknown char throws the reference's string and adds no sample."""
    out = run_spec()
    assert 'spec_restore_gpu ok' in out and 'route: device' in out


@pytest.mark.gpu
def test_encode_device_0_takes_the_js_loop_with_the_same_result():
    out = run_spec(dict(os.environ, BPE_ENCODE_DEVICE='0'))
    assert 'spec_restore_gpu ok' in out and 'route: js loop' in out
