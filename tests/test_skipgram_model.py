"""The skip-gram model on the device (bpe_sgmodel_*, csrc/bpe_sgmodel.hip) against its rule in numpy
float64, dense, from the same fp32 parameters.

Tolerance: the error of an output x is max|x - x64| / max|x64|.  The yardstick is the
same rule in numpy float32 over exactly the cases below (it needs no GPU); the tolerance of a kind is
8 x the largest float32 error over the cases, and never below 1e-6 (16 fp32 ulps)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from bpe_amd import pkg

pytestmark = pytest.mark.gpu

T = getattr(pkg, 'SGM_TILE', 64)
SHAPES = [(1, 1), (3, 2), (T - 1, 50), (T, 64), (T + 1, 65), (2 * T + 3, 50), (3 * T, 256)]
PATTERNS = ['full', 'text', 'sparse']
SCALES = ['unit', 'sixty']
ADAM = dict(lr=0.05, beta1=0.9, beta2=0.999, eps=1e-4)   # (eps well above the fp32 error of a gradient: a
#                                                          well-conditioned step, whatever sign a tiny entry has)
# largest float32-numpy errors over the cases:  loss 1.24e-07  dEin 9.48e-07  db1 1.08e-05  dEout 7.14e-07
# db2 6.31e-07  params after three Adam steps 4.52e-07  ->  8 x each, floored at 1e-6
TOL = {'loss': 1.0e-6, 'dEin': 7.6e-6, 'db1': 8.6e-5, 'dEout': 5.7e-6, 'db2': 5.0e-6, 'params': 3.6e-6}
KINDS = ['loss', 'dEin', 'db1', 'dEout', 'db2']


def rule(params, planes, V, dt=np.float64):
    """(loss, dEin, db1, dEout, db2) of the issue's rule, dense, in dtype dt."""
    Ein, b1, Eout, b2 = [p.astype(dt) for p in params]
    C = np.zeros((V, V), dt)
    C[planes[0], planes[1]] = planes[2]
    n = C.sum(1)
    P = n.sum()
    if P == 0:
        return (dt(0), 0 * Ein, 0 * b1, 0 * Eout, 0 * b2)
    H = Ein + b1
    Z = H @ Eout.T + b2
    m = Z.max(1)
    lse = m + np.log(np.exp(Z - m[:, None]).sum(1))
    G = (n[:, None] * np.exp(Z - lse[:, None]) - C) / P
    dH = G @ Eout
    return ((n @ lse - (C * Z).sum()) / P, dH, dH.sum(0), G.T @ H, G.sum(0))


def make_counts(V, pattern, rng):
    C = np.zeros((V, V), np.int64)
    if pattern == 'full':
        C[:] = rng.integers(1, 6, (V, V))
    elif pattern == 'text':   # the symmetric counts of a short text at window 2
        x = rng.integers(0, V, 4 * V + 8)
        for d in (1, 2):
            np.add.at(C, (x[:-d], x[d:]), 1)
            np.add.at(C, (x[d:], x[:-d]), 1)
    else:   # unsymmetric and sparse: whole empty rows and columns, entries on both sides of every tile edge, one 2^33
        C[np.triu_indices(V, 1)] = rng.integers(1, 9, V * (V - 1) // 2) * (rng.random(V * (V - 1) // 2) < 0.1)
        for b in range(32, V, 32):
            C[b - 1, b - 1], C[b - 1, b], C[b, b - 1] = 2, 3, 5
        r = np.arange(V)
        C[(r % 32 == 10) | ((V < 32) & (r == 1)), :] = 0
        C[:, (r % 32 == 20) | ((V < 32) & (r == 2))] = 0
        if V == 3:
            C[2, 0] = 7
        C[0, min(1, V - 1)] = 1 << 33   # (a pair the large-logit parameters do not predict: a cell predicted with
        #                                 p ~ 1 makes loss and gradient differences of equal numbers in any fp32)
    t, c = np.nonzero(C)
    return t.astype(np.int32), c.astype(np.int32), C[t, c]


def make_params(V, E, scale, rng):
    a = np.sqrt(0.4 / E) if scale == 'unit' else np.sqrt(5.0 / np.sqrt(E))   # logits within +-1 / of deviation ~5
    Ein, Eout = rng.uniform(-a, a, (V, E)), rng.uniform(-a, a, (V, E))
    b1, b2 = rng.uniform(-0.1, 0.1, E) * a, rng.uniform(-0.1, 0.1, V)
    if scale == 'sixty':   # +-60 along u: a row's maximum in the first column block (even t) or the last (odd t)
        u = np.zeros(E)
        u[0] = 1.0
        Ein[:, 0] = np.where(np.arange(V) % 2 == 0, 7.5, -7.5) - b1[0]
        Eout[0], Eout[V - 1] = 8 * u, -8 * u if V > 1 else 8 * u
    return [x.astype(np.float32) for x in (Ein, b1, Eout, b2)]


def case(V, E, pattern, scale):
    rng = np.random.default_rng(1000 * V + E)
    return make_params(V, E, scale, rng), make_counts(V, pattern, rng)


def rel_err(x, x64):
    den = np.abs(x64).max()   # (a reference that is exactly zero: the absolute error)
    return float(np.abs(np.asarray(x, np.float64) - x64).max() / (den if den else 1.0))


def adam_reference(params, planes, V, steps, dt):
    p = [x.astype(dt) for x in params]
    m, v, losses = [0 * x for x in p], [0 * x for x in p], []
    for k in range(1, steps + 1):
        out = rule(p, planes, V, dt)
        losses.append(float(out[0]))
        for i, g in enumerate(out[1:]):
            m[i] = dt(ADAM['beta1']) * m[i] + dt(1 - ADAM['beta1']) * g
            v[i] = dt(ADAM['beta2']) * v[i] + dt(1 - ADAM['beta2']) * g * g
            p[i] = p[i] - dt(ADAM['lr']) * (m[i] / dt(1 - ADAM['beta1'] ** k)) / (
                np.sqrt(v[i] / dt(1 - ADAM['beta2'] ** k)) + dt(ADAM['eps']))
    return np.concatenate([x.ravel() for x in p]), losses


# (one row and one column have no first and last column block: V = 1 takes the unit scale only)
CASES = [(V, E, p, s) for V, E in SHAPES for p in PATTERNS for s in SCALES if V > 1 or s == 'unit']


@pytest.mark.parametrize('V,E,pattern,scale', CASES)
def test_loss_grad(V, E, pattern, scale):
    params, planes = case(V, E, pattern, scale)
    want = rule(params, planes, V)
    m = pkg.SkipgramModel(0, V, E)
    m.set_params(*params)
    got = m.loss_grad(*planes)
    errs = {k: rel_err(g, w) for k, g, w in zip(KINDS, got, want)}
    print(V, E, pattern, scale, errs)
    again = m.loss_grad(*planes)
    assert all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(got, again))
    assert all(errs[k] <= TOL[k] for k in KINDS), errs
    empty = m.loss_grad([], [], [])
    assert empty[0] == 0 and all(not g.any() for g in empty[1:])
    assert all(np.array_equal(a, b) for a, b in zip(m.get_params(), params))
    m.close()


def test_adam():
    V, E = T + 1, 50
    params, planes = case(V, E, 'text', 'unit')
    want, want_losses = adam_reference(params, planes, V, 3, np.float64)
    m = pkg.SkipgramModel(0, V, E)
    m.set_params(*params)
    losses = [m.adam_step(*planes, **ADAM) for _ in range(3)]
    got = np.concatenate([x.ravel() for x in m.get_params()])
    print('adam', rel_err(got, want), losses, want_losses)
    assert losses[0] > losses[1] > losses[2]
    assert abs(losses[0] - want_losses[0]) <= TOL['loss'] * want_losses[0]
    assert rel_err(got, want) <= TOL['params']
    assert m.stats()['steps'] == 3
    m.close()


def routes_check():
    import torch
    chars = [chr(0x100 + i) for i in range(T + 6)]
    rng = np.random.default_rng(7)
    texts = [''.join(chars[i] for i in rng.integers(0, len(chars), n)) for n in (150, 1, 90)]
    enc = pkg.Encoder(0)
    enc.set_chars({ch: i for i, ch in enumerate(chars)})
    V, E = len(chars), 50
    params, _ = case(V, E, 'text', 'unit')
    m = pkg.SkipgramModel(0, V, E)
    m.set_params(*params)
    host = m.loss_grad(*enc.skipgram_counts_text(texts, 2, 'ids', V))
    units = np.frombuffer(''.join(texts).encode('utf-16-le'), np.int16)
    off = np.concatenate([[0], np.cumsum([len(t) for t in texts])]).astype(np.int64)
    planes = enc.skipgram_counts_text_tensors(torch.from_numpy(units.copy()).cuda(), torch.from_numpy(off).cuda(), 2, 'ids', V)
    dev = m.loss_grad_tensors(*planes)
    assert host[0] == dev[0] and host[0] > 0
    assert all(a.tobytes() == b.cpu().numpy().tobytes() for a, b in zip(host[1:], dev[1:]))
    assert rel_err(host[1], rule(params, [p.cpu().numpy() for p in planes], V)[1]) <= TOL['dEin']
    ids = np.array([V - 1, 0, 5, 5], np.int32)
    assert np.array_equal(m.embed(ids), params[0][ids] + params[1])
    assert np.array_equal(m.embed_tensors(torch.from_numpy(ids).cuda()).cpu().numpy(), params[0][ids] + params[1])
    assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(m.get_params_tensors(), params))
    m.close()
    enc.close()
    return True


def test_routes():
    """In a process of its own that imports torch before libbpe loads (PyTorch sees a device only when its
    HIP runtime is the process's first)."""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([here, os.environ.get('PYTHONPATH', '')]))
    out = subprocess.run([sys.executable, os.path.abspath(__file__), 'routes'], env=env, capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith('routes ok'), out.stdout[-2000:] + out.stderr[-3000:]


@pytest.mark.parametrize('planes,message', [
    (([1, 0], [0, 1], [1, 1]), r'pairs must ascend: \(0, 1\) after \(1, 0\) \(element 1\)'),
    (([0, 1, 1], [2, 1, 1], [1, 1, 1]), r'pair \(1, 1\) is given twice \(element 2\)'),
    (([0, 5], [1, 2], [1, 1]), r'target 5 outside \[0, 5\) \(element 1\)'),
    (([0, 1], [5, 2], [1, 1]), r'context 5 outside \[0, 5\) \(element 0\)'),
    (([0, 1, 2], [1, 2, 3], [1, -4, -1]), r'count -4 is negative \(element 1\)'),
])
def test_errors(planes, message):
    V, E = 5, 3
    params, good = case(V, E, 'full', 'unit')
    m = pkg.SkipgramModel(0, V, E)
    m.set_params(*params)
    m.adam_step(*good, **ADAM)
    before = m.get_params()
    for call in (m.loss_grad, lambda *p: m.adam_step(*p, **ADAM)):
        with pytest.raises(pkg.BpeError, match=message) as e:
            call(*planes)
        assert e.value.code == pkg.ERR_ARG
    with pytest.raises(pkg.BpeError, match='parameters of 4 x 3 given to a model of 5 x 3') as e:
        m.set_params(params[0][:4], params[1], params[2][:4], params[3][:4])
    assert e.value.code == pkg.ERR_ARG
    with pytest.raises(pkg.BpeError, match='are no \\(Ein, b1, Eout, b2\\)'):
        m.set_params(params[0], params[1], params[2], params[3][:4])
    for dim, embed, msg in ((pkg.SKIPGRAM_COUNTS_MAX_DIM + 1, 3, 'dim 16385 outside'), (5, pkg.SGM_MAX_EMBED + 1, 'embed 257 outside')):
        with pytest.raises(pkg.BpeError, match=msg) as e:
            pkg.SkipgramModel(0, dim, embed)
        assert e.value.code == pkg.ERR_ARG
    assert all(np.array_equal(a, b) for a, b in zip(m.get_params(), before)) and m.stats()['steps'] == 1
    # the Adam state too: the second step from here is the second step of an undisturbed model
    fresh = pkg.SkipgramModel(0, V, E)
    fresh.set_params(*params)
    for _ in range(2):
        fresh.adam_step(*good, **ADAM)
    m.adam_step(*good, **ADAM)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(m.get_params(), fresh.get_params()))
    m.close()
    fresh.close()


if __name__ == '__main__' and sys.argv[1:] == ['routes']:
    import torch  # noqa: F401  (before libbpe loads)
    print('routes ok' if routes_check() else 'failed')
