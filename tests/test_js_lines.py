"""The corpus-helper batch methods of the Node drop-in (bpe-tokenizer_amd/js/core.js over
addon/bpe_lines_napi.node): the addon's exports, the methods and their typings on CPU, and on the GPU
the four methods against the same class fed `texts.flatMap(helper)` through the existing string methods
(tests/js/lines_gpu.js)."""
import os
import shutil
import subprocess

import pytest

from bpe_amd import ROOT, pkg

NODE = shutil.which('node')
ADDON_DIR = os.path.join(ROOT, 'bpe-tokenizer_amd', 'addon')
CORE = os.path.join(ROOT, 'bpe-tokenizer_amd', 'js', 'core.js')
METHODS = ('addLinesToCorpusBatch', 'addLinesToCorpusBatchUtf8', 'restoreLinesToCorpusBatch',
           'restoreLinesToCorpusBatchUtf8')

pytestmark = pytest.mark.skipif(NODE is None, reason='node not installed')


def build_addon():
    subprocess.check_call(['make', '-s', '-C', ADDON_DIR])
    if not os.path.exists(os.path.join(ADDON_DIR, 'bpe_lines_napi.node')):
        pytest.skip('no addon (node headers missing)')


def test_lines_addon_builds_and_exports():
    build_addon()
    out = subprocess.check_output([NODE, '-e', "const a=require(process.argv[1]);"
                                   "console.log(Object.keys(a).sort().join(','))",
                                   os.path.join(ADDON_DIR, 'bpe_lines_napi.node')], text=True)
    assert out.strip() == 'addLinesBatch,addLinesUtf8Batch,restoreLinesBatch,restoreLinesUtf8Batch'
    core = subprocess.check_output([NODE, '-e', "const {BPETokenizer}=require(process.argv[1]);"
                                    "console.log(%r.map(k=>typeof BPETokenizer.prototype[k]).join(','))"
                                    % (list(METHODS),), CORE], text=True)
    assert core.strip() == ','.join(['function'] * 4)
    dts = open(os.path.join(ROOT, 'bpe-tokenizer_amd', 'js', 'core.d.ts')).read()
    assert "export type CorpusHelperName = 'linesToCorpus' | 'linesTrimmedToCorpus' | 'fileContentToCorpus'" in dts
    for name in METHODS:
        arg = 'buffers: Array<Buffer | Uint8Array>' if name.endswith('Utf8') else 'texts: string[]'
        assert '%s(%s, helper?: CorpusHelperName): void' % (name, arg) in dts


def test_an_unknown_helper_throws_and_without_a_device_the_methods_fail_with_the_usual_error():
    build_addon()
    script = ("const {BPETokenizer}=require(process.argv[1]);const t=new BPETokenizer();"
              "const arg=k=>k.endsWith('Utf8')?[Buffer.from(' ab\\n')]:[' ab\\n'];"
              "for(const k of %r){for(const h of ['trim',undefined]){"
              "try{t[k](arg(k),h);console.log(k+': no error')}catch(e){console.log(k+': '+e.message)}}}" % (list(METHODS),))
    out = subprocess.run([NODE, '-e', script, CORE], capture_output=True, text=True)
    lines = out.stdout.strip().split('\n')
    assert len(lines) == 8, out.stdout + out.stderr
    for k, name in enumerate(METHODS):
        assert lines[2 * k].startswith(name + ': unknown corpus helper: trim'), lines[2 * k]
        if pkg.device_count() == 0:
            assert 'no HIP device' in lines[2 * k + 1], lines[2 * k + 1]


@pytest.mark.gpu
def test_lines_batch_methods_equal_the_string_methods_on_the_helper_samples():
    """The four methods on files (the golden config's stream with line ends planted, several scripts
    with every kind of whitespace, ill-formed bytes, an empty file) against flatMap(helper) through
    addToCorpus and restoreToCorpus, for the three helpers: toJSON(), corpus_in_code, merges, and one
    unknown-char error string."""
    build_addon()
    out = subprocess.run([NODE, os.path.join(ROOT, 'tests', 'js', 'lines_gpu.js')],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert 'lines_gpu ok' in out.stdout
