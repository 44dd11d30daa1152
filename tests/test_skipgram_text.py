"""The skip-gram model over texts (bpe_sgmodel_embed_texts / _score_texts, csrc/bpe_sgtext.hip.h) against their
rules in numpy float64 from the same fp32 parameters.

Tolerance: the error of an output x is max|x - x64| / max|x64| over a batch.  The yardstick is the
same rule in plain numpy float32 over exactly the cases below (it needs no GPU); the tolerance of a kind is 4 x
the largest float32 error over the cases: both are fp32 sums of at most 3C + 5 terms in different orders (of
(F + 1) C + 3 terms for the one long text of test_long, which has bounds of its own for that).

  kind    float32 numpy   tolerance   kernels on an MI355X
  pool    3.04e-6         1.22e-5     1.69e-6
  score   6.95e-7         2.78e-6     4.86e-7
  long pool    3.84e-5    1.54e-4     9.01e-7
  long score   1.47e-6    5.87e-6     5.38e-7"""
import os
import subprocess
import sys

import numpy as np
import pytest

from bpe_amd import pkg

C, F = getattr(pkg, 'SGM_TEXT_CHUNK', 256), getattr(pkg, 'SGM_TEXT_FOLD', 64)
SHAPES = [(7, 3), (70, 50), (130, 64), (65, 256)]   # the three load widths, the three EP, V on both sides of 64
LENS = [0, 1, 2, C - 1, C, C + 1, 3 * C + 5, 0, 0]  # (the last value of C + 1 has all its pairs across the chunk edge)
LONG = (F + 1) * C + 3   # more than F chunks: they are added in two levels
POOLS = ['sum', 'mean', 'unit']
WINDOWS = [1, 2, 64]
TOL = {'pool': 1.22e-5, 'score': 2.78e-6, 'long pool': 1.54e-4, 'long score': 5.87e-6}
NAMES = ['bpe_sgmodel_embed_texts', 'bpe_sgmodel_embed_texts_device', 'bpe_sgmodel_score_texts',
         'bpe_sgmodel_score_texts_device', 'bpe_sgmodel_get_text_stats', 'bpe_sgmodel_reset_text_stats']
gpu = pytest.mark.gpu


def case(V, E):
    """(params, texts, weights): parameters of magnitude ~0.5 and of one sign, so that no pooled sum is near zero
    by accident; weights with zeros; every value of the text of C + 1 values has weight zero."""
    rng = np.random.default_rng(100 * V + E)
    params = [rng.uniform(0.25, 0.75, s).astype(np.float32) for s in ((V, E), (E,), (V, E), (V,))]
    texts = [rng.integers(0, V, n).astype(np.int32) for n in LENS]
    w = rng.uniform(0.1, 1.0, V).astype(np.float32)
    w[::3] = 0
    texts[5][:] = 3 * rng.integers(0, (V + 2) // 3, C + 1)
    return params, texts, w


def flat(texts, lead=0):
    """(vals, off) with `lead` values that belong to no text (and to no table) in front."""
    off = lead + np.concatenate([[0], np.cumsum([len(t) for t in texts])]).astype(np.int64)
    return np.concatenate([np.full(lead, -7, np.int32)] + list(texts)), off


def pool_rule(params, texts, w, pool, dt=np.float64):
    X = (params[0] + params[1]).astype(dt)
    out = np.zeros((len(texts), X.shape[1]), dt)
    for k, t in enumerate(texts):
        wt = np.ones(len(t), dt) if w is None else w[t].astype(dt)
        s, ws = (wt[:, None] * X[t]).sum(0, dtype=dt), wt.sum(dtype=dt)
        norm = np.sqrt((s * s).sum(dtype=dt))
        scale = {'sum': dt(1), 'mean': 1 / ws if ws else dt(0), 'unit': 1 / norm if norm else dt(0)}[pool]
        out[k] = s * scale
    return out


def score_rule(params, texts, window, dt=np.float64):
    Ein, b1, Eout, b2 = params
    Z = (Ein + b1).astype(dt) @ Eout.astype(dt).T + b2.astype(dt)
    m = Z.max(1, keepdims=True)
    logp = Z - (m + np.log(np.exp(Z - m).sum(1, keepdims=True, dtype=dt)))
    sums, pairs = np.zeros(len(texts), dt), np.zeros(len(texts), np.int64)
    for k, t in enumerate(texts):
        for i in range(len(t)):
            js = [j for j in range(max(0, i - window), min(len(t) - 1, i + window) + 1) if j != i]
            sums[k] += logp[t[i], t[js]].sum(dtype=dt)
            pairs[k] += len(js)
    return sums, pairs


def rel_err(got, want):
    return float(np.abs(np.asarray(got, np.float64) - want).max() / np.abs(want).max())


def model(V, E, params):
    m = pkg.SkipgramModel(0, V, E)
    m.set_params(*params)
    return m


@gpu
@pytest.mark.parametrize('V,E', SHAPES)
def test_pool(V, E):
    params, texts, w = case(V, E)
    m = model(V, E, params)
    for pool in POOLS:
        for wt in (None, w):
            got = m.embed_texts(texts, weights=wt, pool=pool)
            err = rel_err(got, pool_rule(params, texts, wt, pool))
            print('pool', V, E, pool, wt is not None, err)
            assert err <= TOL['pool']
            zero = [k for k, t in enumerate(texts) if len(t) == 0 or (wt is not None and pool != 'sum' and k == 5)]
            assert not got[zero].any() and got[6].any()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(m.get_params(), params)) and m.stats()['steps'] == 0
    m.close()


@gpu
@pytest.mark.parametrize('V,E', SHAPES)
def test_score(V, E):
    params, texts, _ = case(V, E)
    m = model(V, E, params)
    n_pairs = {}
    for window in WINDOWS:
        want, want_pairs = score_rule(params, texts, window)
        n_pairs[window] = int(want_pairs.sum())
        got, pairs = m.score_texts(texts, window=window)
        print('score', V, E, window, rel_err(got, want))
        assert pairs.tolist() == want_pairs.tolist() and rel_err(got, want) <= TOL['score']
        assert not got[[0, 1, 7, 8]].any()
    before = m.query_stats()
    m.score_texts(texts)
    assert m.query_stats() == before and m.stats()['steps'] == 0
    assert all(a.tobytes() == b.tobytes() for a, b in zip(m.get_params(), params))
    st = m.text_stats()
    assert st['calls'] == 4 and st['texts'] == 4 * len(LENS) and st['values'] == 4 * sum(LENS)
    assert st['items'] == 4 * sum(max(1, -(-n // C)) for n in LENS) and st['pairs'] == sum(n_pairs.values()) + n_pairs[2]
    m.close()


@gpu
@pytest.mark.parametrize('V,E', SHAPES)
def test_long(V, E):
    """A text of more than F chunks, alone and behind the short texts: the same bytes, and the rules."""
    params, texts, w = case(V, E)
    long = [np.random.default_rng(V).integers(0, V, LONG).astype(np.int32)]
    m = model(V, E, params)
    for pool in POOLS:
        got = m.embed_texts(long, weights=w, pool=pool)
        err = rel_err(got, pool_rule(params, long, w, pool))
        print('long pool', V, E, pool, err)
        assert err <= TOL['long pool'] and got.tobytes() == m.embed_texts(texts + long, weights=w, pool=pool)[-1:].tobytes()
    (got, pairs), (want, want_pairs) = m.score_texts(long, window=2), score_rule(params, long, 2)
    print('long score', V, E, rel_err(got, want))
    assert pairs.tolist() == want_pairs.tolist() and rel_err(got, want) <= TOL['long score']
    assert got.tobytes() == m.score_texts(texts + long, window=2)[0][-1:].tobytes()
    m.close()


@gpu
@pytest.mark.parametrize('V,E', SHAPES)
def test_batch_independence(V, E):
    """A text's row and sum_logp are the same bytes alone, at either place of the reordered batch with off[0] > 0,
    and on a second run."""
    params, texts, w = case(V, E)
    m = model(V, E, params)
    rows, sums = m.embed_texts(texts, weights=w, pool='unit'), m.score_texts(texts, window=2)[0]
    assert rows.tobytes() == m.embed_texts(texts, weights=w, pool='unit').tobytes()
    assert sums.tobytes() == m.score_texts(texts, window=2)[0].tobytes()
    vals, off = flat(texts[::-1], lead=5)
    assert m.embed_texts(vals, off, weights=w, pool='unit')[::-1].tobytes() == rows.tobytes()
    assert m.score_texts(vals, off, window=2)[0][::-1].tobytes() == sums.tobytes()
    for k, t in enumerate(texts):
        assert m.embed_texts([t], weights=w, pool='unit').tobytes() == rows[k].tobytes()
        assert m.score_texts([t], window=2)[0].tobytes() == sums[k].tobytes()
    m.close()


def routes_check():
    """Host forms against the `_tensors` forms, byte for byte; a refused device call leaves its output alone."""
    import torch
    for V, E in SHAPES:
        params, texts, w = case(V, E)
        m = model(V, E, params)
        vals, off = flat(texts[::-1], lead=5)
        dv, do, dw = torch.from_numpy(vals).cuda(), torch.from_numpy(off).cuda(), torch.from_numpy(w).cuda()
        for pool in POOLS:
            assert m.embed_texts(vals, off, w, pool).tobytes() == m.embed_texts_tensors(dv, do, dw, pool).cpu().numpy().tobytes()
        host, dev = m.score_texts(vals, off, 64), m.score_texts_tensors(dv, do, 64)
        assert all(h.tobytes() == d.cpu().numpy().tobytes() for h, d in zip(host, dev))
        out = torch.full((len(texts), E), 7.0, device='cuda')
        dv[5] = V
        with pytest.raises(pkg.BpeError, match=r'value %d outside \[0, %d\) \(text 2, value 0\)' % (V, V)):
            m.embed_texts_tensors(dv, do, dw, 'sum', out=out)
        assert bool((out == 7.0).all())
        empty = m.embed_texts_tensors(dv[:0], do[:1])
        assert tuple(empty.shape) == (0, E)
        m.close()
    return True


@gpu
def test_routes():
    """In a process of its own that imports torch before libbpe loads (PyTorch sees a device only when its
    HIP runtime is the process's first)."""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([here, os.environ.get('PYTHONPATH', '')]))
    out = subprocess.run([sys.executable, os.path.abspath(__file__), 'routes'], env=env, capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith('routes ok'), out.stdout[-2000:] + out.stderr[-3000:]


@gpu
def test_errors():
    V, E = 70, 50
    params, texts, w = case(V, E)
    m = model(V, E, params)
    vals, off = flat(texts, lead=3)
    # two offenders, whole chunks and workgroups of the check apart: the smallest flat position is named
    for (k0, i0, v0), (k1, i1, v1) in (((3, 7, V), (6, 2 * C + 9, -1)), ((4, 1, -1), (6, 3 * C, V))):
        bad = vals.copy()
        bad[off[k0] + i0], bad[off[k1] + i1] = v0, v1
        msg = r'skip-gram model value %d outside \[0, %d\) \(text %d, value %d\)' % (v0, V, k0, i0)
        for call in (lambda: m.embed_texts(bad, off, w), lambda: m.score_texts(bad, off)):
            with pytest.raises(pkg.BpeError, match=msg) as e:
                call()
            assert e.value.code == pkg.ERR_ARG
    down = off.copy()
    down[4] = down[3] - 1
    for call, msg in ((lambda: m.embed_texts(vals, down), 'offsets must not decrease'),
                      (lambda: m.score_texts(vals, down), 'offsets must not decrease'),
                      (lambda: m.embed_texts(vals, off, pool='median'), 'skip-gram model pool -1 is none of'),
                      (lambda: m.embed_texts(vals, off, pool=3), 'skip-gram model pool 3 is none of'),
                      (lambda: m.score_texts(vals, off, window=0), r'skip-gram model window 0 outside \[1, 64\]'),
                      (lambda: m.score_texts(vals, off, window=65), r'skip-gram model window 65 outside \[1, 64\]')):
        with pytest.raises(pkg.BpeError, match=msg) as e:
            call()
        assert e.value.code == pkg.ERR_ARG
    assert m.embed_texts([]).shape == (0, E) and [len(x) for x in m.score_texts([])] == [0, 0]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(m.get_params(), params)) and m.stats()['steps'] == 0
    m.close()


def test_names():
    assert all(n in pkg.C_API and hasattr(pkg.lib(), n) for n in NAMES)


if __name__ == '__main__' and sys.argv[1:] == ['routes']:
    import torch  # noqa: F401  (before libbpe loads)
    print('routes ok' if routes_check() else 'failed')
