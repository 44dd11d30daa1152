"""The dense-count form of the skip-gram model's training steps (bpe_sgmodel_set_counts_form,
csrc/bpe_sgdense.hip.h) against the rules of test_skipgram_model (full softmax) and test_skipgram_sgns
(negative sampling) in numpy float64, over those files' cases, within those files' tolerances.

The negative-sampling file has no (T - 1, 50) and (T, 64).  The float32 rule over them (all its patterns, sets
and scales, on the CPU) errs by at most loss 1.68e-7, dEin 4.78e-7, db1 8.07e-7, dEout 3.96e-7, db2 3.99e-7;
by that file's yardstick (8 x, never below 1e-6) these two shapes get SGNS_ADDED_TOL, tighter than its TOL."""
import os
import subprocess
import sys

import numpy as np
import pytest

import test_skipgram_model as SM
import test_skipgram_sgns as SN
from bpe_amd import pkg

pytestmark = pytest.mark.gpu

T = SM.T
SHAPES = [(1, 1), (3, 2), (T - 1, 50), (T, 64), (T + 1, 65), (2 * T + 3, 50), (3 * T, 256)]
CASES = [(SM, V, E, p, s) for V, E in SHAPES for p in SM.PATTERNS for s in SM.SCALES if V > 1 or s == 'unit']
CASES += [(SN, V, E, p, s, n) for V, E in SHAPES for p in SN.PATTERNS for s in SN.SCALES for n in SN.SETS
          if V > 1 or s == 'unit']
SGNS_ADDED_TOL = {'loss': 1.35e-6, 'dEin': 3.9e-6, 'db1': 6.5e-6, 'dEout': 3.2e-6, 'db2': 3.2e-6}


def setup(mod, V, E, *rest):
    """(params, planes, the rule's extra arguments, loss_grad, adam_step) of a case of either file."""
    params, planes, *nset = mod.case(V, E, *rest)
    if mod is SM:
        return params, planes, (), (lambda m, *p: m.loss_grad(*p)), (lambda m, *p: m.adam_step(*p, **SM.ADAM))
    return (params, planes, tuple(nset), (lambda m, *p: m.sgns_loss_grad(*p, *nset[0], neg_k=SN.KAPPA)),
            (lambda m, *p: m.sgns_adam_step(*p, *nset[0], neg_k=SN.KAPPA, **SN.ADAM)))


def same_bytes(a, b):
    return all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize('mod,V,E,rest', [(c[0], c[1], c[2], c[3:]) for c in CASES],
                         ids=['-'.join([c[0].__name__[14:]] + [str(x) for x in c[1:]]) for c in CASES])
def test_dense_loss_grad(mod, V, E, rest):
    params, planes, extra, loss_grad, _ = setup(mod, V, E, *rest)
    want = mod.rule(params, planes, V, *extra)
    n64 = (V + T - 1) // T
    tol = SGNS_ADDED_TOL if mod is SN and (V, E) not in SN.SHAPES else mod.TOL
    m = pkg.SkipgramModel(0, V, E)
    m.set_params(*params)
    for splits in (0, 1, 3):   # at 2T + 3 and 3T: one split holds all three tiles, three hold one each
        m.set_counts_form('dense', splits)
        got = loss_grad(m, *planes)
        st = m.dense_stats()
        errs = {k: mod.rel_err(g, w) for k, g, w in zip(mod.KINDS, got, want)}
        print(mod.__name__, V, E, rest, splits, st['last_splits'], errs)
        assert st['last_form'] == 'dense' and 1 <= st['last_splits'] <= n64
        assert not splits or st['last_splits'] == min(splits, n64)
        assert same_bytes(got, loss_grad(m, *planes))
        assert all(errs[k] <= tol[k] for k in mod.KINDS), errs
    empty = loss_grad(m, [], [], [])
    assert empty[0] == 0 and all(not g.any() for g in empty[1:])
    assert all(np.array_equal(a, b) for a, b in zip(m.get_params(), params))
    m.close()


@pytest.mark.parametrize('mod,case', [(SM, (T + 1, 50, 'text', 'unit')), (SN, SN.ADAM_CASE)], ids=['model', 'sgns'])
def test_dense_adam(mod, case):
    params, planes, extra, _, adam_step = setup(mod, *case)
    want, want_losses = mod.adam_reference(params, planes, case[0], *extra, 3, np.float64)
    m = pkg.SkipgramModel(0, *case[:2])
    m.set_params(*params)
    m.set_counts_form('dense')
    losses = [adam_step(m, *planes) for _ in range(3)]
    got = np.concatenate([x.ravel() for x in m.get_params()])
    print('adam', mod.rel_err(got, want), losses, want_losses)
    assert losses[0] > losses[1] > losses[2]
    assert abs(losses[0] - want_losses[0]) <= mod.TOL['loss'] * want_losses[0]
    assert mod.rel_err(got, want) <= mod.TOL['params']
    assert m.stats()['steps'] == 3 and m.dense_stats()['dense_calls'] == 3
    m.close()


def test_forms():
    V, E = 3 * T, 256
    params, full = SM.case(V, E, 'full', 'unit')
    sparse = SM.case(V, E, 'sparse', 'unit')[1]
    # theta was measured as 1/64 and the file's sparse case fills 4.8 % of the cells: its first 500 elements
    # (planes still, 1.4 %) are the case below theta; the whole of it lies above, with the full case
    below = tuple(x[:500] for x in sparse)
    assert len(below[0]) < pkg.SGM_DENSE_THETA * V * V <= len(sparse[0]) < len(full[0])
    m, fresh = pkg.SkipgramModel(0, V, E), pkg.SkipgramModel(0, V, E)
    m.set_params(*params)
    fresh.set_params(*params)
    m.set_counts_form('dense')
    m.set_counts_form('csr')   # ... is the default, untouched
    assert same_bytes(m.loss_grad(*sparse), fresh.loss_grad(*sparse)) and m.dense_stats()['last_form'] == 'csr'
    m.set_counts_form('auto')
    for planes, form in ((full, 'dense'), (below, 'csr'), (sparse, 'dense'), (below, 'csr'), (full, 'dense')):
        m.loss_grad(*planes)
        assert m.dense_stats()['last_form'] == form
    for bad in (('sideways', 0), (7, 0), ('csr', 257), ('csr', -1)):
        with pytest.raises(pkg.BpeError, match='counts form|splits') as e:
            m.set_counts_form(*bad)
        assert e.value.code == pkg.ERR_ARG
    m.loss_grad(*full)
    assert m.dense_stats()['last_form'] == 'dense'   # (still 'auto')
    # a bad plane under the dense form: the message of the CSR form, parameters and Adam state unchanged
    m.set_counts_form('dense')
    fresh.set_counts_form('dense')
    m.adam_step(*full, **SM.ADAM)
    before = m.get_params()
    for call in (m.loss_grad, lambda *p: m.adam_step(*p, **SM.ADAM)):
        with pytest.raises(pkg.BpeError, match=r'pairs must ascend: \(0, 1\) after \(1, 0\) \(element 1\)') as e:
            call([1, 0], [0, 1], [1, 1])
        assert e.value.code == pkg.ERR_ARG
    assert same_bytes(m.get_params(), before) and m.stats()['steps'] == 1
    for _ in range(2):
        fresh.adam_step(*full, **SM.ADAM)
    m.adam_step(*full, **SM.ADAM)
    assert same_bytes(m.get_params(), fresh.get_params())
    m.close()
    fresh.close()


def routes_check():
    import torch
    for mod, case in ((SM, (T + 1, 50, 'text', 'unit')), (SN, SN.ADAM_CASE)):
        params, planes, extra, loss_grad, adam_step = setup(mod, *case)
        dev = [torch.from_numpy(x).cuda() for x in planes + tuple(extra[0] if extra else ())]
        neg = dict(neg_k=SN.KAPPA) if extra else {}
        m = pkg.SkipgramModel(0, *case[:2])
        m.set_counts_form('dense')
        m.set_params(*params)
        host = loss_grad(m, *planes)
        got = (m.sgns_loss_grad_tensors if extra else m.loss_grad_tensors)(*dev, **neg)
        assert host[0] == got[0] and host[0] > 0 and same_bytes(host[1:], [x.cpu().numpy() for x in got[1:]])
        adam_step(m, *planes)
        after = m.get_params()
        m.set_params(*params)
        m.reset_optimizer()
        (m.sgns_adam_step_tensors if extra else m.adam_step_tensors)(*dev, **neg, **mod.ADAM)
        assert same_bytes(after, [x.cpu().numpy() for x in m.get_params_tensors()])
        assert m.dense_stats()['dense_calls'] == m.dense_stats()['calls'] == 4
        m.close()
    return True


def test_dense_routes():
    """In a process of its own that imports torch before libbpe loads (PyTorch sees a device only when its
    HIP runtime is the process's first)."""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([here, os.environ.get('PYTHONPATH', '')]))
    out = subprocess.run([sys.executable, os.path.abspath(__file__), 'routes'], env=env, capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith('routes ok'), out.stdout[-2000:] + out.stderr[-3000:]


if __name__ == '__main__' and sys.argv[1:] == ['routes']:
    import torch  # noqa: F401  (before libbpe loads)
    print('routes ok' if routes_check() else 'failed')
