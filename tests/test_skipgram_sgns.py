"""Skip-gram with negative sampling on the device (bpe_sgmodel_sgns_*, csrc/bpe_sgns.hip.h) against its
rule in numpy float64, dense, from the same fp32 parameters.

Tolerance: the error of an output x is max|x - x64| / max|x64|.  The yardstick is the
same rule with the same stable formulas in numpy float32 over exactly the cases below (it needs no GPU);
the tolerance of a kind is 8 x the largest float32 error over the cases, and never below 1e-6.

  kind     float32 numpy   tolerance   kernels on an MI355X
  loss     1.46e-6         1.16e-5     1.44e-6
  dEin     2.40e-6         1.92e-5     4.21e-6
  db1      2.39e-6         1.91e-5     4.19e-6
  dEout    2.41e-6         1.92e-5     2.29e-6
  db2      2.39e-6         1.91e-5     2.28e-6
  params   4.13e-7         3.3e-6      4.00e-7     (after three Adam steps)
(The float32 errors come from the logits near +-60, where exp(-|z|) carries |z| ulps of z.)"""
import os
import subprocess
import sys

import numpy as np
import pytest

from bpe_amd import pkg

pytestmark = pytest.mark.gpu

T = getattr(pkg, 'SGM_TILE', 64)
W = getattr(pkg, 'SGNS_ROWS', 32)
SHAPES = [(1, 1), (3, 2), (W - 1, 50), (W + 1, 64), (T + 1, 65), (2 * T + 3, 50), (3 * T, 256)]
PATTERNS = ['text', 'sparse']
SETS = ['none', 'one', 'some', 'exact']
SCALES = ['unit', 'sixty']
KAPPA = 5.0
ADAM = dict(lr=0.05, beta1=0.9, beta2=0.999, eps=1e-4)   # (the model test's, for its reason: eps well above the
#                                                          fp32 error of a gradient)
TOL = {'loss': 1.16e-5, 'dEin': 1.92e-5, 'db1': 1.91e-5, 'dEout': 1.92e-5, 'db2': 1.91e-5, 'params': 3.3e-6}
KINDS = ['loss', 'dEin', 'db1', 'dEout', 'db2']


def rule(params, planes, V, neg, dt=np.float64):
    """(loss, dEin, db1, dEout, db2) of the issue's rule, dense, in dtype dt."""
    Ein, b1, Eout, b2 = [p.astype(dt) for p in params]
    C = np.zeros((V, V), dt)
    C[planes[0], planes[1]] = planes[2]
    n = C.sum(1)
    P = n.sum()
    if P == 0:
        return (dt(0), 0 * Ein, 0 * b1, 0 * Eout, 0 * b2)
    omega = np.zeros(V, dt)
    omega[neg[0]] = dt(KAPPA) * neg[1].astype(dt)
    H = Ein + b1
    Z = H @ Eout.T + b2
    e = np.exp(-np.abs(Z))
    hi, lo, l1p = 1 / (1 + e), e / (1 + e), np.log1p(e)
    N = n[:, None] * omega[None, :]
    L = -((C * (np.minimum(Z, 0) - l1p)).sum() + (N * (np.minimum(-Z, 0) - l1p)).sum()) / P
    G = (N * np.where(Z >= 0, hi, lo) - C * np.where(Z >= 0, lo, hi)) / P
    dH = G @ Eout
    return (L, dH, dH.sum(0), G.T @ H, G.sum(0))


def make_counts(V, pattern, rng):
    C = np.zeros((V, V), np.int64)
    if pattern == 'text':   # the symmetric counts of a short text at window 2
        x = rng.integers(0, V, 4 * V + 8)
        for d in (1, 2):
            np.add.at(C, (x[:-d], x[d:]), 1)
            np.add.at(C, (x[d:], x[:-d]), 1)
    else:   # unsymmetric and sparse: entries on both sides of every tile edge, a row and a column of more than 32
        #     entries (tiles span rows, a row spans tiles), whole empty rows and columns, one 2^33
        C[np.triu_indices(V, 1)] = rng.integers(1, 9, V * (V - 1) // 2) * (rng.random(V * (V - 1) // 2) < 0.1)
        for b in range(W, V, W):
            C[b - 1, b - 1], C[b - 1, b], C[b, b - 1] = 2, 3, 5
        if V > W:
            C[5, :], C[:, 7] = rng.integers(1, 4, V), rng.integers(1, 4, V)
        r = np.arange(V)
        C[(r % 32 == 10) | ((V < 32) & (r == 1)), :] = 0
        C[:, (r % 32 == 20) | ((V < 32) & (r == 2))] = 0
        if V == 3:
            C[2, 0] = 7
        C[0, min(1, V - 1)] = 1 << 33
    t, c = np.nonzero(C)
    return t.astype(np.int32), c.astype(np.int32), C[t, c]


def make_params(V, E, scale, rng):
    a = np.sqrt(0.4 / E) if scale == 'unit' else np.sqrt(5.0 / np.sqrt(E))   # logits within +-1 / of deviation ~5
    Ein, Eout = rng.uniform(-a, a, (V, E)), rng.uniform(-a, a, (V, E))
    b1, b2 = rng.uniform(-0.1, 0.1, E) * a, rng.uniform(-0.1, 0.1, V)
    if scale == 'sixty':   # z = +-60 in the first and the last column: both branches of sigma and ls saturate
        Ein[:, 0] = np.where(np.arange(V) % 2 == 0, 7.5, -7.5) - b1[0]
        Eout[0], Eout[V - 1] = 0, 0
        Eout[0, 0], Eout[V - 1, 0] = 8, -8
    return [x.astype(np.float32) for x in (Ein, b1, Eout, b2)]


def make_set(V, kind, planes, rng):
    """(ids int32 ascending, weights float32) of the negative set."""
    if kind == 'none':
        ids, w = [], []
    elif kind == 'one':
        ids, w = [V // 2], [1.0]
    elif kind == 'some':   # 33 ids (all of a smaller V), among them the positives 0, 1, V - 1 of some row
        ids = np.union1d([0, min(1, V - 1), V - 1], rng.permutation(V)[:min(33, V)])[:min(33, V)]
        w = rng.integers(1, 4, len(ids)) / 64.0
    else:   # the exact expected objective: every id, weighted by the noise distribution
        q = np.bincount(planes[1], planes[2].astype(np.float64), V) ** 0.75
        ids, w = np.arange(V), q / max(q.sum(), 1e-300)
    return np.asarray(ids, np.int32), np.asarray(w, np.float32)


def case(V, E, pattern, scale, neg):
    rng = np.random.default_rng(1000 * V + E)
    params, planes = make_params(V, E, scale, rng), make_counts(V, pattern, rng)
    return params, planes, make_set(V, neg, planes, rng)


def rel_err(x, x64):
    den = np.abs(x64).max()   # (a reference that is exactly zero: the absolute error)
    return float(np.abs(np.asarray(x, np.float64) - x64).max() / (den if den else 1.0))


def adam_reference(params, planes, V, neg, steps, dt):
    p = [x.astype(dt) for x in params]
    m, v, losses = [0 * x for x in p], [0 * x for x in p], []
    for k in range(1, steps + 1):
        out = rule(p, planes, V, neg, dt)
        losses.append(float(out[0]))
        for i, g in enumerate(out[1:]):
            m[i] = dt(ADAM['beta1']) * m[i] + dt(1 - ADAM['beta1']) * g
            v[i] = dt(ADAM['beta2']) * v[i] + dt(1 - ADAM['beta2']) * g * g
            p[i] = p[i] - dt(ADAM['lr']) * (m[i] / dt(1 - ADAM['beta1'] ** k)) / (
                np.sqrt(v[i] / dt(1 - ADAM['beta2'] ** k)) + dt(ADAM['eps']))
    return np.concatenate([x.ravel() for x in p]), losses


# (one row and one column have no first and last column: V = 1 takes the unit scale only)
CASES = [(V, E, p, n, s) for V, E in SHAPES for p in PATTERNS for n in SETS for s in SCALES if V > 1 or s == 'unit']
ADAM_CASE = (T + 1, 50, 'text', 'unit', 'some')


@pytest.mark.parametrize('V,E,pattern,neg,scale', CASES)
def test_loss_grad(V, E, pattern, neg, scale):
    params, planes, nset = case(V, E, pattern, scale, neg)
    want = rule(params, planes, V, nset)
    m = pkg.SkipgramModel(0, V, E)
    m.set_params(*params)
    got = m.sgns_loss_grad(*planes, *nset, neg_k=KAPPA)
    errs = {k: rel_err(g, w) for k, g, w in zip(KINDS, got, want)}
    print(V, E, pattern, neg, scale, errs)
    again = m.sgns_loss_grad(*planes, *nset, neg_k=KAPPA)
    assert all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(got, again))
    assert all(errs[k] <= TOL[k] for k in KINDS), errs
    if neg == 'none':   # ... and so is neg_k = 0 with any set
        zero_k = m.sgns_loss_grad(*planes, [0], [1.0], neg_k=0.0)
        assert all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(got, zero_k))
    empty = m.sgns_loss_grad([], [], [], *nset, neg_k=KAPPA)
    assert empty[0] == 0 and all(not g.any() for g in empty[1:])
    assert all(np.array_equal(a, b) for a, b in zip(m.get_params(), params))
    m.close()


def test_adam():
    V, E = ADAM_CASE[:2]
    params, planes, nset = case(*ADAM_CASE)
    want, want_losses = adam_reference(params, planes, V, nset, 3, np.float64)
    m = pkg.SkipgramModel(0, V, E)
    m.set_params(*params)
    losses = [m.sgns_adam_step(*planes, *nset, neg_k=KAPPA, **ADAM) for _ in range(3)]
    got = np.concatenate([x.ravel() for x in m.get_params()])
    print('adam', rel_err(got, want), losses, want_losses)
    assert losses[0] > losses[1] > losses[2]
    assert abs(losses[0] - want_losses[0]) <= TOL['loss'] * want_losses[0]
    assert rel_err(got, want) <= TOL['params']
    assert m.stats()['steps'] == 3 and m.sgns_stats()['calls'] == 3 and m.sgns_stats()['negatives'] == 3 * len(nset[0])
    m.close()


def routes_check():
    import torch
    V, E = T + 1, 64
    params, planes, _ = case(V, E, 'text', 'unit', 'none')
    m = pkg.SkipgramModel(0, V, E)
    q = m.noise(*planes)
    assert np.allclose(q, case(V, E, 'text', 'unit', 'exact')[2][1], rtol=1e-6, atol=0)
    nset = m.sample_negatives(q, 40, seed=3)
    assert np.all(np.diff(nset[0]) > 0) and abs(nset[1].sum() - 1) < 1e-6
    dev = [torch.from_numpy(x).cuda() for x in planes + nset]
    for w_host, w_dev in ((nset[1], dev[4]), (None, None)):   # (given weights; 1/S each)
        m.set_params(*params)
        m.reset_optimizer()
        host = m.sgns_loss_grad(*planes, nset[0], w_host, neg_k=KAPPA)
        got = m.sgns_loss_grad_tensors(*dev[:4], w_dev, neg_k=KAPPA)
        assert host[0] == got[0] and host[0] > 0
        assert all(a.tobytes() == b.cpu().numpy().tobytes() for a, b in zip(host[1:], got[1:]))
        m.sgns_adam_step(*planes, nset[0], w_host, neg_k=KAPPA, **ADAM)
        after = m.get_params()
        m.set_params(*params)
        m.reset_optimizer()
        m.sgns_adam_step_tensors(*dev[:4], w_dev, neg_k=KAPPA, **ADAM)
        assert all(a.tobytes() == b.cpu().numpy().tobytes() for a, b in zip(after, m.get_params_tensors()))
    m.close()
    return True


def test_routes():
    """In a process of its own that imports torch before libbpe loads (PyTorch sees a device only when its
    HIP runtime is the process's first)."""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([here, os.environ.get('PYTHONPATH', '')]))
    out = subprocess.run([sys.executable, os.path.abspath(__file__), 'routes'], env=env, capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith('routes ok'), out.stdout[-2000:] + out.stderr[-3000:]


@pytest.mark.parametrize('ids,weights,neg_k,message', [
    ([1, 3, 2], None, 5.0, r'negative ids must ascend: 2 after 3 \(element 2\)'),
    ([1, 1], None, 5.0, r'negative ids must ascend: 1 after 1 \(element 1\)'),
    ([0, 5], None, 5.0, r'negative id 5 outside \[0, 5\) \(element 1\)'),
    ([-1, 2], None, 5.0, r'negative id -1 outside \[0, 5\) \(element 0\)'),
    ([0, 2, 4], [0.5, -0.25, -1.0], 5.0, r'negative weight -0.25 is negative or not finite \(element 1\)'),
    ([0, 2], [0.5, float('nan')], 5.0, r'negative weight nan is negative or not finite \(element 1\)'),
    ([0, 2], [float('inf'), 0.5], 5.0, r'negative weight inf is negative or not finite \(element 0\)'),
    ([0, 2], None, -1.0, r'neg_k -1 is negative or not finite'),
    ([0, 2], None, float('inf'), r'neg_k inf is negative or not finite'),
    ([0, 1, 2, 3, 4, 5], None, 5.0, r'negatives 6 outside \[0, 5\]'),
])
def test_errors(ids, weights, neg_k, message):
    V, E = 5, 3
    params, good, nset = case(V, E, 'text', 'unit', 'some')
    m = pkg.SkipgramModel(0, V, E)
    m.set_params(*params)
    m.sgns_adam_step(*good, *nset, neg_k=KAPPA, **ADAM)
    before = m.get_params()
    for call in (m.sgns_loss_grad, lambda *p, **k: m.sgns_adam_step(*p, **k, **ADAM)):
        with pytest.raises(pkg.BpeError, match=message) as e:
            call(*good, ids, weights, neg_k=neg_k)
        assert e.value.code == pkg.ERR_ARG
    with pytest.raises(pkg.BpeError, match=r'pairs must ascend: \(0, 1\) after \(1, 0\) \(element 1\)'):
        m.sgns_adam_step([1, 0], [0, 1], [1, 1], *nset, neg_k=KAPPA, **ADAM)
    assert all(np.array_equal(a, b) for a, b in zip(m.get_params(), before)) and m.stats()['steps'] == 1
    # the Adam state too: the second step from here is the second step of an undisturbed model
    fresh = pkg.SkipgramModel(0, V, E)
    fresh.set_params(*params)
    for _ in range(2):
        fresh.sgns_adam_step(*good, *nset, neg_k=KAPPA, **ADAM)
    m.sgns_adam_step(*good, *nset, neg_k=KAPPA, **ADAM)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(m.get_params(), fresh.get_params()))
    m.close()
    fresh.close()


if __name__ == '__main__' and sys.argv[1:] == ['routes']:
    import torch  # noqa: F401  (before libbpe loads)
    print('routes ok' if routes_check() else 'failed')
