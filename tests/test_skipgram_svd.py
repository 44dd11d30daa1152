"""PPMI and its truncated SVD on the device (bpe_sgmodel_ppmi*, csrc/bpe_svd.hip.h) against the rule in numpy
float64 from the same planes and the same explicit Omega, over the count patterns of test_skipgram_sgns.py.
The reference takes orth as numpy.linalg.qr and the eigenproblem as numpy.linalg.eigh; only quantities that do
not depend on the sign or rotation of singular vectors are compared: sigma, Ein Eout^T and Ein Ein^T.

Tolerance: the error of x is max|x - x64| / max|x64|.  The yardstick is the same rule in
numpy float32 over exactly the cases of test_ppmi and test_svd (it needs no GPU); the tolerance of a kind is 8 x
the largest float32 error over the cases, and never below 1e-6.

  kind     float32 numpy   tolerance   kernels on an MI355X
  ppmi     4.59e-7         3.67e-6     0 (the same bytes in every case)
  sigma    1.93e-7         1.54e-6     8.68e-8
  recon    3.78e-6         3.03e-5     3.54e-6     (Ein Eout^T)
  gram     1.61e-6         1.29e-5     5.47e-7     (Ein Ein^T)
`python tests/test_skipgram_svd.py yardstick` prints the float32 column and the smallest gap; no case was unstable
in float32.  Every case has a float64 gap sigma_E / sigma_{E+1} >= 1.05 (asserted below);
SEEDS lists the cases whose seed was moved for it.  Every sigma_i is also held to sigma_i of numpy.linalg.svd of the
dense matrix times (1 + the sigma tolerance); no case on the device exceeds it."""
import os
import subprocess
import sys

import numpy as np
import pytest

from bpe_amd import pkg
from test_skipgram_glove import same, with_zeros
from test_skipgram_sgns import ADAM, make_counts, rel_err

gpu = pytest.mark.gpu

SHAPES = [(17, 1, 0), (33, 3, 13), (65, 8, 16), (70, 50, 14), (130, 64, 0), (131, 50, 78)]   # L = 16 16 32 64 64 128
PATTERNS = ['text', 'sparse']
SETTINGS = [(1.0, 1.0, 0.5), (5.0, 0.75, 0.0), (1.0, 0.75, 1.0)]   # shift, cds, gamma
TOL = {'ppmi': 3.67e-6, 'sigma': 1.54e-6, 'recon': 3.03e-5, 'gram': 1.29e-5}
GAP = 1.05
# (V, pattern) or (V, pattern, shift, cds) -> the seed of the planes and Omega where the default leaves the
# reference's sigma_E / sigma_{E+1} below GAP
SEEDS = {(33, 'text'): 5, (65, 'text'): 114, (65, 'sparse'): 4, (70, 'text'): 3, (131, 'sparse'): 23,
         (131, 'text', 1.0, 1.0): 3426, (131, 'text', 5.0, 0.75): 159, (131, 'text', 1.0, 0.75): 9068}
NAMES = ['bpe_sgmodel_ppmi', 'bpe_sgmodel_ppmi_device', 'bpe_sgmodel_ppmi_svd', 'bpe_sgmodel_ppmi_svd_device',
         'bpe_sgmodel_get_svd_stats', 'bpe_sgmodel_reset_svd_stats']
METHODS = ['ppmi', 'ppmi_tensors', 'ppmi_svd', 'ppmi_svd_tensors', 'svd_stats', 'reset_svd_stats']


def width(E, oversample):
    return (E + oversample + 15) // 16 * 16


def case(V, E, oversample, pattern, shift=None, cds=None):
    rng = np.random.default_rng(SEEDS.get((V, pattern, shift, cds), SEEDS.get((V, pattern), 1000 * V + E)))
    planes = make_counts(V, pattern, rng)
    return planes, rng.standard_normal((V, width(E, oversample))).astype(np.float32)


def ppmi_rule(planes, V, shift, cds, dt=np.float64):
    """m of every element of the planes, in dtype dt, rounded to float32."""
    t, c, k = planes
    C = np.zeros((V, V), np.int64)
    C[t, c] = k
    r, kc = C.sum(1), C.sum(0)
    Z = (kc[kc > 0].astype(dt) ** dt(cds)).sum()
    with np.errstate(divide='ignore'):
        m = np.log(k.astype(dt)) - np.log(r[t].astype(dt)) - dt(cds) * np.log(kc[c].astype(dt)) + np.log(Z) - np.log(dt(shift))
    return np.where(k > 0, np.maximum(m, 0), 0).astype(np.float32)


def dense(planes, V, shift, cds):
    M = np.zeros((V, V), np.float64)
    M[planes[0], planes[1]] = ppmi_rule(planes, V, shift, cds)
    return M


def svd_rule(M, omega, E, power_iters, gamma, dt=np.float64):
    """(all L sigma, Ein, Eout) of the issue's rule on the dense PPMI matrix, in dtype dt."""
    M = M.astype(dt)
    Q = np.linalg.qr(M @ omega.astype(dt))[0]
    for _ in range(power_iters):
        Q = np.linalg.qr(M @ np.linalg.qr(M.T @ Q)[0])[0]
    B = M.T @ Q
    lam, Wh = np.linalg.eigh(B.T @ B)
    lam, Wh = lam[::-1], Wh[:, ::-1]
    sig = np.sqrt(np.maximum(lam, 0))
    inv = np.where(sig > 1e-7 * sig[0], 1 / np.where(sig > 0, sig, 1), 0).astype(dt)
    U, Vm = Q @ Wh, (B @ Wh) * inv
    return sig, U[:, :E] * sig[:E] ** dt(gamma), Vm[:, :E] * sig[:E] ** dt(1 - gamma)


def kinds(sig, Ein, Eout):
    Ein, Eout = np.asarray(Ein, np.float64), np.asarray(Eout, np.float64)
    return {'sigma': np.asarray(sig, np.float64)[:Ein.shape[1]], 'recon': Ein @ Eout.T, 'gram': Ein @ Ein.T}


def gap_ok(sig, E):
    return len(sig) == E or sig[E] == 0 or sig[E - 1] / sig[E] >= GAP


def run(m, planes, **kw):
    sig = m.ppmi_svd(*planes, **kw)
    Ein, b1, Eout, b2 = m.get_params()
    return sig, Ein, Eout, b1, b2


@gpu
@pytest.mark.parametrize('shift,cds,gamma', SETTINGS)
@pytest.mark.parametrize('pattern', PATTERNS)
@pytest.mark.parametrize('V,E,oversample', SHAPES)
def test_ppmi(V, E, oversample, pattern, shift, cds, gamma):
    planes, _ = case(V, E, oversample, pattern, shift, cds)
    want = ppmi_rule(planes, V, shift, cds)
    m = pkg.SkipgramModel(0, V, E)
    got = m.ppmi(*planes, shift=shift, cds=cds)
    err = rel_err(got, want.astype(np.float64))
    print(V, pattern, shift, cds, err)
    assert err <= TOL['ppmi']
    zeros = with_zeros(planes, V)
    gz = m.ppmi(*zeros, shift=shift, cds=cds)
    assert not gz[zeros[2] == 0].any() and gz[zeros[2] > 0].tobytes() == got.tobytes()
    st = m.svd_stats()
    assert st['calls'] == 2 and st['cells'] == 2 * len(got) and st['positive_cells'] == 2 * int((got > 0).sum())
    m.close()


@gpu
@pytest.mark.parametrize('shift,cds,gamma', SETTINGS)
@pytest.mark.parametrize('power_iters', [0, 2])
@pytest.mark.parametrize('pattern', PATTERNS)
@pytest.mark.parametrize('V,E,oversample', SHAPES)
def test_svd(V, E, oversample, pattern, power_iters, shift, cds, gamma):
    planes, omega = case(V, E, oversample, pattern, shift, cds)
    M = dense(planes, V, shift, cds)
    want = svd_rule(M, omega, E, power_iters, gamma)
    assert gap_ok(want[0], E), want[0][E - 1:E + 1]
    m = pkg.SkipgramModel(0, V, E)
    opts = dict(shift=shift, cds=cds, gamma=gamma, oversample=oversample, power_iters=power_iters, omega=omega)
    sig, Ein, Eout, b1, b2 = run(m, planes, **opts)
    got, ref = kinds(sig, Ein, Eout), kinds(*want)
    errs = {k: rel_err(got[k], ref[k]) for k in ref}
    print(V, E, oversample, pattern, power_iters, shift, cds, gamma, errs, m.svd_stats())
    assert all(errs[k] <= TOL[k] for k in errs), errs
    true = np.linalg.svd(M, compute_uv=False)[:E]
    assert (sig <= true * (1 + TOL['sigma'])).all(), (sig / true - 1).max()
    assert not b1.any() and not b2.any() and m.svd_stats()['L'] == width(E, oversample)
    # the same bytes again, and from planes with zero-count elements spliced in
    assert same(run(m, planes, **opts), (sig, Ein, Eout, b1, b2))
    assert same(run(m, with_zeros(planes, V), **opts), (sig, Ein, Eout, b1, b2))
    m.close()


def low_rank_case():
    V, E, oversample = 40, 8, 24
    planes, omega = case(V, E, oversample, 'text')
    keep = np.isin(planes[0], [3, 9, 17, 18, 31])
    return V, E, oversample, tuple(p[keep] for p in planes), omega


@gpu
@pytest.mark.parametrize('rank', ['five', 'full'])
def test_seeds(rank):
    """The seeded Omega: the same bytes for the same seed, other bytes for another.  On the planes of rank 5 < L
    every start spans the whole range, so sigma agrees to rounding; on planes of rank above L two starts differ by
    what two power iterations leave, so there each sigma is held to the true values from above only."""
    V, E, oversample, planes, _ = low_rank_case() if rank == 'five' else (130, 64, 0) + case(130, 64, 0, 'text')
    m = pkg.SkipgramModel(0, V, E)
    a = run(m, planes, oversample=oversample, power_iters=2, seed=7)
    assert same(a, run(m, planes, oversample=oversample, power_iters=2, seed=7))
    b = run(m, planes, oversample=oversample, power_iters=2, seed=8)
    print('seeds', rank, rel_err(b[0], a[0]))
    assert a[1].tobytes() != b[1].tobytes() and a[0].tobytes() != b[0].tobytes()
    true = np.linalg.svd(dense(planes, V, 1.0, 1.0), compute_uv=False)[:E]
    assert all((s <= true * (1 + TOL['sigma'])).all() for s in (a[0], b[0]))
    assert rank == 'full' or rel_err(b[0], a[0]) <= TOL['sigma']
    m.close()


@gpu
def test_low_rank_and_empty():
    V, E, oversample, planes, omega = low_rank_case()
    want = svd_rule(dense(planes, V, 1.0, 1.0), omega, E, 2, 0.5)
    m = pkg.SkipgramModel(0, V, E)
    sig, Ein, Eout, _, _ = run(m, planes, oversample=oversample, power_iters=2, omega=omega)
    got, ref = kinds(sig, Ein, Eout), kinds(*want)
    errs = {k: rel_err(got[k], ref[k]) for k in ref}
    print('low rank', errs, sig, m.svd_stats())
    assert m.svd_stats()['dropped_columns'] > 0
    assert np.isfinite(Ein).all() and np.isfinite(Eout).all() and np.isfinite(sig).all()
    assert not sig[5:].any() and sig[4] > 0   # (dropped columns are exact zeros from B on)
    assert all(errs[k] <= TOL[k] for k in errs), errs
    sig = m.ppmi_svd([], [], [], oversample=oversample)
    assert not sig.any() and not any(x.any() for x in m.get_params())
    m.close()


@gpu
def test_model_left_usable():
    V, E = 70, 50
    planes, omega = case(V, E, 14, 'text')
    m = pkg.SkipgramModel(0, V, E)
    rng = np.random.default_rng(5)
    m.set_params(*[rng.standard_normal(s).astype(np.float32) for s in m._shapes()])
    for _ in range(2):
        m.glove_adam_step(*planes, **ADAM)
    m.neighbors([0, 1], 5)
    m.ppmi_svd(*planes, oversample=14, omega=omega)
    Ein, b1, Eout, b2 = m.get_params()
    assert not b1.any() and not b2.any() and m.stats()['steps'] == 0
    ids = np.arange(V, dtype=np.int32)
    X = Ein.astype(np.float64)
    n = np.linalg.norm(X, axis=1, keepdims=True)
    X = X / np.where(n > 0, n, 1)   # (a token the planes never name has a zero row: its cosines are 0)
    S = X @ X.T
    np.fill_diagonal(S, -np.inf)
    got, scores = m.neighbors(ids, 5)
    top = np.sort(S, axis=1)[:, ::-1][:, :5]
    assert np.abs(scores - top).max() <= 1e-5 and np.abs(S[ids[:, None], got] - top).max() <= 1e-5
    # the next step is a first step: the same as on a fresh model given the parameters
    fresh = pkg.SkipgramModel(0, V, E)
    fresh.set_params(Ein, b1, Eout, b2)
    fresh.set_target_bias(m.get_target_bias())
    assert m.glove_adam_step(*planes, **ADAM) == fresh.glove_adam_step(*planes, **ADAM)
    assert same(m.get_params() + (m.get_target_bias(),), fresh.get_params() + (fresh.get_target_bias(),))
    m.close()
    fresh.close()


def routes_check():
    import torch
    V, E = 70, 50
    planes, omega = case(V, E, 14, 'sparse')
    dev = [torch.from_numpy(x).cuda() for x in planes]
    m = pkg.SkipgramModel(0, V, E)
    host = run(m, planes, oversample=14, power_iters=2, omega=omega)
    sig = m.ppmi_svd_tensors(*dev, oversample=14, power_iters=2, omega=torch.from_numpy(omega).cuda())
    p = [x.cpu().numpy() for x in m.get_params_tensors()]
    assert same(host, (sig, p[0], p[2], p[1], p[3]))
    assert m.ppmi(*planes, cds=0.75).tobytes() == m.ppmi_tensors(*dev, cds=0.75).cpu().numpy().tobytes()
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
@pytest.mark.parametrize('V,bad,message', [
    (70, dict(shift=0.0), r'skip-gram model shift 0 is not positive or not finite'),
    (70, dict(cds=0.0), r'skip-gram model cds 0 outside \(0, 1\]'),
    (70, dict(cds=1.5), r'skip-gram model cds 1.5 outside \(0, 1\]'),
    (70, dict(gamma=-0.5), r'skip-gram model gamma -0.5 outside \[0, 1\]'),
    (70, dict(gamma=float('nan')), r'skip-gram model gamma nan outside \[0, 1\]'),
    (70, dict(oversample=-1), r'skip-gram model oversample -1 is negative'),
    (70, dict(power_iters=-2), r'skip-gram model power_iters -2 is negative'),
    (70, dict(oversample=80), r'skip-gram model svd width 144 \(embed 50 \+ oversample 80, in sixteens\) above the limit 128'),
    (60, dict(oversample=14), r'skip-gram model svd width 64 \(embed 50 \+ oversample 14, in sixteens\) above dim 60'),
])
def test_errors(V, bad, message):
    E = 50
    planes, _ = case(V, E, 14, 'text')
    m = pkg.SkipgramModel(0, V, E)
    m.glove_adam_step(*planes, **ADAM)
    before = m.get_params() + (m.get_target_bias(),)
    with pytest.raises(pkg.BpeError, match=message) as e:
        m.ppmi_svd(*planes, **dict(dict(oversample=14), **bad))
    assert e.value.code == pkg.ERR_ARG
    if set(bad) & {'shift', 'cds'}:
        with pytest.raises(pkg.BpeError, match=message):
            m.ppmi(*planes, **bad)
    assert same(m.get_params() + (m.get_target_bias(),), before) and m.stats()['steps'] == 1
    m.close()


def test_exports():
    assert all(n in pkg.C_API and hasattr(pkg.lib(), n) for n in NAMES)
    assert all(callable(getattr(pkg.SkipgramModel, n, None)) for n in METHODS) and pkg.SVD_MAX_L == 128


def yardstick():
    """The float32 column of the table above and the smallest gap, over the cases of test_ppmi and test_svd."""
    worst, gap = dict.fromkeys(TOL, 0.0), np.inf
    for (V, E, ov) in SHAPES:
        for pattern in PATTERNS:
            for shift, cds, gamma in SETTINGS:
                planes, omega = case(V, E, ov, pattern, shift, cds)
                m64 = ppmi_rule(planes, V, shift, cds).astype(np.float64)
                worst['ppmi'] = max(worst['ppmi'], rel_err(ppmi_rule(planes, V, shift, cds, np.float32), m64))
                for power_iters in (0, 2):
                    want = svd_rule(dense(planes, V, shift, cds), omega, E, power_iters, gamma)
                    a, b = kinds(*svd_rule(dense(planes, V, shift, cds), omega, E, power_iters, gamma, np.float32)), kinds(*want)
                    worst.update({k: max(worst[k], rel_err(a[k], b[k])) for k in b})
                    gap = min(gap, want[0][E - 1] / want[0][E] if len(want[0]) > E and want[0][E] > 0 else np.inf)
    print(worst, {k: max(1e-6, 8 * v) for k, v in worst.items()}, 'smallest gap %.4f' % gap)


if __name__ == '__main__' and sys.argv[1:] == ['yardstick']:
    yardstick()
if __name__ == '__main__' and sys.argv[1:] == ['routes']:
    import torch  # noqa: F401  (before libbpe loads)
    print('routes ok' if routes_check() else 'failed')
