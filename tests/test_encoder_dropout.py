"""BPE-dropout on the device (csrc/bpe_dropout.hip.h, include/bpe.h "encoding with dropout") against
`rule`, a plain restatement of the sequential rule: M scans in list order, a Python-int mix64 coin per
site.  The rule is exact, so every comparison is equality of integer lists."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from bpe_amd import ROOT, pkg
from test_encoder_split import random_texts, trained_merges

M64 = (1 << 64) - 1
CAP = pkg.ENCODE_LDS_TOKENS
SEED = 0xFEDCBA9876543210
LENGTHS = [1, 2, 3, 128, 129, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193, 16384]


def mix64(z):
    z ^= z >> 30
    z = z * 0xBF58476D1CE4E5B9 & M64
    z ^= z >> 27
    z = z * 0x94D049BB133111EB & M64
    return z ^ z >> 31


def stream(seed, t, s, S):
    return mix64((seed + 0x9E3779B97F4A7C15 * (t * S + s + 1)) & M64)


def coin(st, i, r):
    return mix64(st ^ ((i << 16 | r) & M64)) >> 32


def rule(text, merges, p, seed, t, s, S):
    """Sample s of S of text t: for every merge in list order one scan left to right; a site that is
    not dropped merges and the scan goes on behind the new token.  (numpy only finds the sites.)"""
    st, thr = stream(seed, t, s, S), int(p * 4294967296.0)
    tok, pos = np.asarray(text, np.int64), np.arange(len(text))
    for r, (a, b, c) in enumerate(merges):
        taken, free = [], 0
        for q in np.flatnonzero((tok[:-1] == a) & (tok[1:] == b)).tolist():
            if q >= free and coin(st, int(pos[q]), r) >= thr:
                taken.append(q)
                free = q + 2
        if taken:
            tok[taken] = c
            keep = np.ones(len(tok), bool)
            keep[np.asarray(taken) + 1] = False
            tok, pos = tok[keep], pos[keep]
    return tok.tolist()


def rule_batch(texts, merges, p, seed, text_base, S):
    return [[rule(t, merges, p, seed, text_base + k, s, S) for s in range(S)] for k, t in enumerate(texts)]


def as_lists(got):
    return [[s.tolist() for s in text] for text in got]


@pytest.fixture(scope='module')
def lists():
    """alphabet -> (merges, x): a trained list, then (x, x) -> y and (y, y) -> z over a fresh id x."""
    out = {}
    for alphabet in (2, 12):
        m = trained_merges(np.random.default_rng(alphabet), alphabet, 40, 400, max_iterations=40)
        x = alphabet + len(m)
        out[alphabet] = (m + [(x, x, x + 1), (x + 1, x + 1, x + 2)], x)
    return out


def raw(enc, texts, samples, p, text_base=0, seed=SEED):
    """bpe_encode_dropout_batch into canary-filled outputs -> (rc, out, out_off)."""
    off = np.zeros(len(texts) + 1, np.int64)
    np.cumsum([len(t) for t in texts], out=off[1:])
    ids = np.concatenate([np.asarray(t, np.int32) for t in texts] + [np.zeros(1, np.int32)])
    out = np.full(int(off[-1]) * max(samples, 1) + 1, -7, np.int32)
    oo = np.full(len(texts) * max(samples, 1) + 1, -7, np.int64)
    i32p, i64p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)
    rc = pkg.lib().bpe_encode_dropout_batch(enc._enc, ids.ctypes.data_as(i32p), off.ctypes.data_as(i64p), len(texts),
                                            samples, p, seed, text_base, out.ctypes.data_as(i32p), oo.ctypes.data_as(i64p))
    return rc, out, oo


def refused(enc, texts, why):
    rc, out, oo = raw(enc, texts, 2, 0.5)
    assert rc == pkg.ERR_STATE and 'no dropout form for text 0: ' + why in pkg.last_error()
    assert (out == -7).all() and (oo == -7).all()


# ---- GPU ------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_p0_is_encode_and_p1_is_the_input(lists):
    merges, x = lists[12]
    texts = random_texts(np.random.default_rng(1), 12, [0, 1, 5, 300, 3000]) + [np.full(777, x, np.int32)]
    enc = pkg.Encoder(0, merges)
    want = [t.tolist() for t in enc.encode(texts)]
    assert as_lists(enc.encode_dropout(texts, 0.0, samples=2)) == [[w, w] for w in want]
    assert as_lists(enc.encode_dropout(texts, 1.0, seed=SEED)) == [[t.tolist()] for t in texts]
    st = enc.dropout_stats()
    assert (st['calls'], st['texts'], st['samples']) == (2, 12, 18) and st['tokens_out'] > 0 and st['steps'] > 0
    enc.reset_dropout_stats()
    assert enc.dropout_stats()['calls'] == 0
    enc.close()


@pytest.mark.gpu
@pytest.mark.parametrize('alphabet', [2, 12])
@pytest.mark.parametrize('p', [0.1, 0.5, 0.9])
def test_the_rule(lists, alphabet, p):
    """Every launch shape's capacity from both sides, random texts and runs of one id (the parity
    chain with dropped sites, at segment edges of every shape)."""
    merges, x = lists[alphabet]
    texts = random_texts(np.random.default_rng(int(p * 10)), alphabet, LENGTHS) + [np.full(l, x, np.int32) for l in LENGTHS]
    enc = pkg.Encoder(0, merges)
    got = as_lists(enc.encode_dropout(texts, p, samples=3, seed=SEED, text_base=1 << 33))
    enc.close()
    want = rule_batch(texts, merges, p, SEED, 1 << 33, 3)
    for k in range(len(texts)):
        assert got[k] == want[k], (k, len(texts[k]))


@pytest.mark.gpu
def test_table_placement_and_batch_position(lists):
    """Four texts alone (few workgroups: the table in LDS) and inside a batch of 300 (the table in
    HBM); text k under text_base b is text 0 under text_base b + k."""
    merges, _x = lists[12]
    rng = np.random.default_rng(3)
    batch = random_texts(rng, 12, rng.integers(0, 700, 300).tolist())
    four = random_texts(rng, 12, [200, 333, 600, 5000])
    batch[100:104] = four
    enc = pkg.Encoder(0, merges)
    inside = as_lists(enc.encode_dropout(batch, 0.3, samples=3, seed=SEED, text_base=5))
    assert as_lists(enc.encode_dropout(four, 0.3, samples=3, seed=SEED, text_base=105)) == inside[100:104]
    for k in (0, 7, 103, 299):
        assert as_lists(enc.encode_dropout([batch[k]], 0.3, samples=3, seed=SEED, text_base=5 + k)) == [inside[k]]
    assert inside[101] == rule_batch([four[1]], merges, 0.3, SEED, 106, 3)[0]
    enc.close()


@pytest.mark.gpu
def test_long_texts(lists):
    """About 40 000 tokens with an id no merge knows planted less than 16 384 apart: cut there under
    'split', with sites named by their place in the text.  What has no dropout form is refused."""
    merges, x = lists[12]
    text = random_texts(np.random.default_rng(4), 12, [40001])[0]
    text[9000::9000] = x + 5
    runs = np.full(CAP + 1000, x, np.int32)
    short = np.arange(5, dtype=np.int32)
    enc = pkg.Encoder(0, merges, long_texts='split')
    got = as_lists(enc.encode_dropout([short, text], 0.4, samples=2, seed=SEED, text_base=9))
    assert got == rule_batch([short, text], merges, 0.4, SEED, 9, 2)
    assert enc.split_stats()['texts_split'] == 1
    rc, out, oo = raw(enc, [short, runs], 2, 0.5)
    assert rc == pkg.ERR_STATE and 'no dropout form for text 1: no safe boundary' in pkg.last_error()
    assert (out == -7).all() and (oo == -7).all()
    enc.set_long_texts('replay')
    refused(enc, [text], 'longer than BPE_ENCODE_LDS_TOKENS tokens on the replay route')
    enc.close()
    enc = pkg.Encoder(0, [(0, 1, 12), (12, 2, 0)])   # (0 is made after it was an input)
    refused(enc, [short], 'the merge list is not one the rank-greedy form takes')
    enc.close()


def text_forms_check(merges, device_form=False):
    """The text forms against the id form on the mapped chars; with device_form the device
    form against the host form (torch's HIP runtime must be the process's first: see test_text_forms)."""
    rng = np.random.default_rng(5)
    abc = 'abcdefghij\U0001F600é'
    texts = [''.join(abc[i] for i in rng.integers(0, 12, l)) for l in (0, 1, 7, 400, 2500)]
    ids = [[abc.index(ch) for ch in t] for t in texts]
    tvi = np.random.default_rng(6).permutation(12 + len(merges) + 3).astype(np.int32)
    enc = pkg.Encoder(0, merges)
    enc.set_chars({ch: i for i, ch in enumerate(abc)})
    enc.set_vector_index(tvi)
    args = dict(samples=2, seed=SEED, text_base=3)
    want = as_lists(enc.encode_dropout(ids, 0.5, **args))
    assert as_lists(enc.encode_text_dropout(texts, 0.5, kind='ids', **args)) == want
    vec = enc.encode_text_dropout(texts, 0.5, **args)
    assert as_lists(vec) == [[tvi[s].tolist() for s in text] for text in want]
    with pytest.raises(pkg.BpeError, match=r'unknown token, char: U\+007A \(text 1, unit 2\)'):
        enc.encode_text_dropout(['ab', 'abz'], 0.5, **args)
    if device_form:
        import torch
        units = np.concatenate([pkg._units(t) for t in texts]).astype(np.int16)
        off = np.cumsum([0] + [len(pkg._units(t)) for t in texts])
        vals, oo = enc.encode_text_dropout_tensors(torch.from_numpy(units).cuda(), torch.from_numpy(off).cuda(), 0.5, **args)
        assert vals.cpu().tolist() == [v for text in vec for s in text for v in s.tolist()]
        assert oo.cpu().tolist() == np.cumsum([0] + [len(s) for text in vec for s in text]).tolist()
    enc.close()


@pytest.mark.gpu
def test_text_forms(lists):
    """Here the host forms; then again with the device form in a process of its own that imports
    torch before libbpe loads (PyTorch sees a device only when its HIP runtime is the process's first)."""
    text_forms_check(lists[12][0])
    pytest.importorskip('torch')
    out = subprocess.run([sys.executable, '-c', 'import torch, sys; sys.path[:0] = %r; import test_encoder_dropout as t; '
                          't.text_forms_check(%r, True); print("device form ok")' % (sys.path, lists[12][0])],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith('device form ok'), out.stdout[-2000:] + out.stderr[-3000:]


@pytest.mark.gpu
@pytest.mark.parametrize('bad', [dict(p=-0.01), dict(p=1.5), dict(p=float('nan')), dict(samples=0), dict(text_base=-1)])
def test_arguments(lists, bad):
    enc = pkg.Encoder(0, lists[12][0])
    with pytest.raises(pkg.BpeError) as e:
        enc.encode_dropout([[0, 1, 2]], **{'p': 0.5, **bad})
    assert e.value.code == pkg.ERR_ARG
    enc.close()


# ---- CPU ------------------------------------------------------------------------------------------

def test_the_rule_header_on_the_host(tmp_path):
    """csrc/bpe_dropout_rule.h as a stand-alone program (with -fsanitize=address,undefined where the
    toolchain links it): its streams, coins and dropped counts are the restatement's, and the dropped
    share of N coins lies within 4 sqrt(p (1 - p) / N) of p."""
    exe = str(tmp_path / 'rule')
    cmd = ['g++', '-std=c++17', '-O1', '-g', '-I', os.path.join(ROOT, 'bpe-tokenizer_amd', 'csrc'), '-o', exe,
           os.path.join(ROOT, 'tests', 'dropout_rule_main.cc')]
    san = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-static-libasan', '-static-libubsan']
    if subprocess.run(cmd + san, capture_output=True).returncode != 0:
        built = subprocess.run(cmd, capture_output=True, text=True)
        assert built.returncode == 0, built.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and not run.stderr, run.stderr[-3000:]
    seen = {'stream': 0, 'coin': 0, 'share': 0}
    for line in run.stdout.splitlines():
        what, *f = line.split()
        seen[what] += 1
        if what == 'stream':
            assert stream(*map(int, f[:4])) == int(f[4]), line
        elif what == 'coin':
            assert coin(*map(int, f[:3])) == int(f[3]), line
        else:
            p, thr, n, dropped = float(f[0]), int(f[1]), int(f[2]), int(f[3])
            st = stream(SEED, 77, 1, 3)
            assert thr == int(p * 4294967296.0) and n == 100000
            assert dropped == sum(coin(st, i // 8, i % 8) < thr for i in range(n)), line
            assert abs(dropped / n - p) <= 4 * (p * (1 - p) / n) ** 0.5, line
    assert seen == {'stream': 64, 'coin': 64 * 24, 'share': 4}


def test_package_exports():
    for name in ('encode_dropout', 'encode_dropout_flat', 'encode_text_dropout', 'encode_text_dropout_flat',
                 'encode_text_dropout_tensors', 'dropout_stats', 'reset_dropout_stats'):
        assert hasattr(pkg.Encoder, name), name
    for name in ('bpe_encode_dropout_batch', 'bpe_encode_dropout_text_batch', 'bpe_encode_dropout_text_batch_device',
                 'bpe_encoder_get_dropout_stats', 'bpe_encoder_reset_dropout_stats'):
        assert name in pkg.C_API and hasattr(pkg.lib(), name), name
    assert [f[0] for f in pkg.DropoutStats._fields_] == ['calls', 'texts', 'samples', 'tokens_in', 'tokens_out',
                                                         'steps', 'kernel_ms']
