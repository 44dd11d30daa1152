"""GloVe on the device (bpe_sgmodel_glove_*, csrc/bpe_glove.hip.h) against its rule in numpy float64 from the
same fp32 parameters, over the count patterns and the magnitudes of test_skipgram_sgns.py.

Tolerance: the error of an output x is max|x - x64| / max|x64|.  The yardstick is the
same rule in numpy float32 over exactly the cases below (it needs no GPU); the tolerance of a kind is 8 x the
largest float32 error over the cases, and never below 1e-6.

  kind     float32 numpy   tolerance   kernels on an MI355X
  loss     2.76e-7         2.21e-6     1.60e-7
  dEin     4.60e-7         3.68e-6     2.77e-7
  db1      4.85e-7         3.88e-6     5.07e-7
  dEout    4.07e-7         3.26e-6     2.53e-7
  db2      3.51e-7         2.81e-6     2.11e-7
  dbt      1.72e-7         1.38e-6     2.92e-7
  params   9.06e-8         1.0e-6      6.25e-8     (after three Adam steps)"""
import os
import subprocess
import sys

import numpy as np
import pytest

from bpe_amd import pkg
from test_skipgram_sgns import ADAM, make_counts, make_params, rel_err

pytestmark = pytest.mark.gpu

R = getattr(pkg, 'GLOVE_RUN', 64)
SHAPES = [(1, 1), (3, 2), (R - 1, 50), (R + 1, 64), (R + 1, 65), (2 * R + 3, 50), (3 * R, 256)]
PATTERNS = ['text', 'sparse']
SCALES = ['unit', 'large']
WEIGHTS = [(100.0, 0.75), (2.0, 0.75), (2.0, 0.0)]   # cells all under the cap, on both sides of it, f = 1
TOL = {'loss': 2.21e-6, 'dEin': 3.68e-6, 'db1': 3.88e-6, 'dEout': 3.26e-6, 'db2': 2.81e-6, 'dbt': 1.38e-6, 'params': 1e-6}
KINDS = ['loss', 'dEin', 'db1', 'dEout', 'db2', 'dbt']


def rule(params, planes, V, x_max, alpha, dt=np.float64):
    """(loss, dEin, db1, dEout, db2, dbt) of the issue's rule, dense, in dtype dt."""
    Ein, b1, Eout, b2, bt = [p.astype(dt) for p in params]
    cell = planes[2] > 0
    t, c, k = [p[cell] for p in planes]
    N = len(k)
    if N == 0:
        return (dt(0), 0 * Ein, 0 * b1, 0 * Eout, 0 * b2, 0 * bt)
    ell = np.log(k.astype(np.float64)).astype(np.float32).astype(dt)
    f = np.minimum(1.0, (k / x_max) ** alpha).astype(np.float32).astype(dt)
    H = Ein + b1
    r = (H[t] * Eout[c]).sum(1) + b2[c] + bt[t] - ell
    G = np.zeros((V, V), dt)
    G[t, c] = f * r / dt(N)
    dH = G @ Eout
    return ((f * r * r).sum() / dt(2 * N), dH, dH.sum(0), G.T @ H, G.sum(0), G.sum(1))


def case(V, E, pattern, scale):
    rng = np.random.default_rng(1000 * V + E)
    params, planes = make_params(V, E, scale, rng), make_counts(V, pattern, rng)
    return params + [rng.uniform(-0.1, 0.1, V).astype(np.float32)], planes


def with_zeros(planes, V):
    """The planes with up to 40 zero-count elements spliced in among the cells, in order."""
    C = np.zeros((V, V), np.int64)
    C[planes[0], planes[1]] = planes[2]
    free = np.flatnonzero(C.ravel() == 0)[::7][:40]
    keys = np.union1d(planes[0].astype(np.int64) * V + planes[1], free)
    return (keys // V).astype(np.int32), (keys % V).astype(np.int32), C.ravel()[keys]


def adam_reference(params, planes, V, steps, dt):
    p = [x.astype(dt) for x in params]
    m, v, losses = [0 * x for x in p], [0 * x for x in p], []
    for k in range(1, steps + 1):
        out = rule(p, planes, V, 100.0, 0.75, dt)
        losses.append(float(out[0]))
        for i, g in enumerate(out[1:]):
            m[i] = dt(ADAM['beta1']) * m[i] + dt(1 - ADAM['beta1']) * g
            v[i] = dt(ADAM['beta2']) * v[i] + dt(1 - ADAM['beta2']) * g * g
            p[i] = p[i] - dt(ADAM['lr']) * (m[i] / dt(1 - ADAM['beta1'] ** k)) / (
                np.sqrt(v[i] / dt(1 - ADAM['beta2'] ** k)) + dt(ADAM['eps']))
    return np.concatenate([x.ravel() for x in p]), losses


def model(V, E, params):
    m = pkg.SkipgramModel(0, V, E)
    m.set_params(*params[:4])
    m.set_target_bias(params[4])
    return m


def same(a, b):
    return all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize('x_max,alpha', WEIGHTS)
@pytest.mark.parametrize('scale', SCALES)
@pytest.mark.parametrize('pattern', PATTERNS)
@pytest.mark.parametrize('V,E', SHAPES)
def test_loss_grad(V, E, pattern, scale, x_max, alpha):
    params, planes = case(V, E, pattern, scale)
    want = rule(params, planes, V, x_max, alpha)
    m = model(V, E, params)
    got = m.glove_loss_grad(*planes, x_max=x_max, alpha=alpha)
    errs = {k: rel_err(g, w) for k, g, w in zip(KINDS, got, want)}
    print(V, E, pattern, scale, x_max, alpha, errs)
    assert same(got, m.glove_loss_grad(*planes, x_max=x_max, alpha=alpha))
    assert all(errs[k] <= TOL[k] for k in KINDS), errs
    zeros = with_zeros(planes, V)
    assert same(got, m.glove_loss_grad(*zeros, x_max=x_max, alpha=alpha))
    empty = m.glove_loss_grad([], [], [], x_max=x_max, alpha=alpha)
    assert empty[0] == 0 and all(not g.any() for g in empty[1:])
    assert same(m.get_params() + (m.get_target_bias(),), params)
    m.close()


def test_adam():
    V, E = R + 1, 50
    params, planes = case(V, E, 'text', 'unit')
    want, want_losses = adam_reference(params, planes, V, 3, np.float64)
    m = model(V, E, params)
    losses = [m.glove_adam_step(*planes, **ADAM) for _ in range(3)]
    bt = m.get_target_bias()
    got = np.concatenate([x.ravel() for x in m.get_params() + (bt,)])
    print('adam', rel_err(got, want), losses, want_losses)
    assert losses[0] > losses[1] > losses[2]
    assert abs(losses[0] - want_losses[0]) <= TOL['loss'] * want_losses[0]
    assert rel_err(got, want) <= TOL['params']
    assert m.stats()['steps'] == 3 and m.glove_stats()['calls'] == 3
    m.adam_step(*planes, **ADAM)   # the softmax step knows nothing of bt
    assert m.stats()['steps'] == 4 and m.get_target_bias().tobytes() == bt.tobytes()
    m.close()


def routes_check():
    import torch
    V, E = R + 1, 64
    params, planes = case(V, E, 'text', 'unit')
    dev = [torch.from_numpy(x).cuda() for x in planes]
    m = model(V, E, params)
    m.set_target_bias_tensors(torch.from_numpy(params[4]).cuda())
    assert m.get_target_bias().tobytes() == params[4].tobytes() == m.get_target_bias_tensors().cpu().numpy().tobytes()
    host = m.glove_loss_grad(*planes, x_max=2.0)
    got = m.glove_loss_grad_tensors(*dev, x_max=2.0)
    assert host[0] == got[0] and host[0] > 0 and same(host[1:], [x.cpu().numpy() for x in got[1:]])
    assert m.glove_adam_step(*planes, x_max=2.0, **ADAM) == host[0]
    after = m.get_params() + (m.get_target_bias(),)
    m.set_params(*params[:4])
    m.set_target_bias(params[4])
    m.reset_optimizer()
    assert m.glove_adam_step_tensors(*dev, x_max=2.0, **ADAM) == host[0]
    assert same(after, [x.cpu().numpy() for x in m.get_params_tensors() + (m.get_target_bias_tensors(),)])
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


@pytest.mark.parametrize('bad,message', [
    (dict(x_max=0.0), r'skip-gram model x_max 0 is not positive or not finite'),
    (dict(x_max=float('inf')), r'skip-gram model x_max inf is not positive or not finite'),
    (dict(alpha=-1.0), r'skip-gram model alpha -1 is negative or not finite'),
    (dict(alpha=float('nan')), r'skip-gram model alpha nan is negative or not finite'),
    (dict(bt=6), r'skip-gram model target bias of 6 given to a model of 5'),
    (dict(planes=([1, 0], [0, 1], [1, 1])), r'skip-gram model pairs must ascend: \(0, 1\) after \(1, 0\) \(element 1\)'),
])
def test_errors(bad, message):
    V, E = 5, 3
    params, good = case(V, E, 'text', 'unit')
    m = model(V, E, params)
    m.glove_adam_step(*good, **ADAM)
    before = m.get_params() + (m.get_target_bias(),)
    bad = dict(bad)
    planes = bad.pop('planes', good)
    calls = ((lambda: m.set_target_bias(np.ones(bad['bt'])),) if 'bt' in bad else
             (lambda: m.glove_loss_grad(*planes, **bad), lambda: m.glove_adam_step(*planes, **bad, **ADAM)))
    for call in calls:
        with pytest.raises(pkg.BpeError, match=message) as e:
            call()
        assert e.value.code == pkg.ERR_ARG
    assert same(m.get_params() + (m.get_target_bias(),), before) and m.stats()['steps'] == 1
    # the Adam state too: the second step from here is the second step of an undisturbed model
    fresh = model(V, E, params)
    for _ in range(2):
        fresh.glove_adam_step(*good, **ADAM)
    m.glove_adam_step(*good, **ADAM)
    assert same(m.get_params() + (m.get_target_bias(),), fresh.get_params() + (fresh.get_target_bias(),))
    m.close()
    fresh.close()


if __name__ == '__main__' and sys.argv[1:] == ['routes']:
    import torch  # noqa: F401  (before libbpe loads)
    print('routes ok' if routes_check() else 'failed')
