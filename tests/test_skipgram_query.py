"""The queries of the skip-gram model (bpe_sgmodel_neighbors / _neighbors_vectors / _predict,
csrc/bpe_sgquery.hip.h) against their rule in numpy float64 from the same fp32 parameters, ordered by
np.lexsort((ids, -scores)).

Exact cases: integer-valued parameters (|X| <= 3, E <= 256: every partial sum is an integer below 2^24, so
fp32 is exact in any order); ids and dot scores must equal the reference, ties included.
Float cases: the error of a kind is max|x - x64| / max|x64|; the yardstick is the same rule
in numpy float32 over exactly the cases below (CPU only), the tolerance 8 x its largest error, never below
1e-6.  Largest float32-numpy errors:  cosine 7.87e-07  prob 4.64e-07  lse 1.08e-07  ->  TOL below.
The kernels' largest errors over the same cases on an MI355X:  cosine 6.2e-07  prob 9.3e-07  lse 1.6e-07."""
import os
import subprocess
import sys

import numpy as np
import pytest

from bpe_amd import pkg

pytestmark = pytest.mark.gpu

ONE_SPLIT_N = 64 * 256   # query tiles of 64 that alone cover the machine's 256 CUs: the host chooses one split
# (V, E, n, k) around the key tile (32), the query tile (32 per wave, 64 per workgroup), the E classes and k
SHAPES = [(1, 1, 1, 1), (3, 2, 3, 5), (31, 50, 31, 4), (32, 64, 33, 32), (33, 65, 65, 1), (65, 50, 1, 64),
          (131, 256, 130, 10), (65, 3, ONE_SPLIT_N, 2)]
TOL = {'cosine': 6.3e-6, 'prob': 3.7e-6, 'lse': 1.0e-6}
FORMS = ['ids', 'vectors', 'predict']


def rule(params, form, query, metric, k, dt=np.float64):
    """-> (ids[n][k], values[n][k], lse[n] or None, the n x V matrix of values) of the issue's rule in dtype dt."""
    X = (params[0] + params[1]).astype(dt)   # fl32(Ein + b1), the row `embed` returns
    Q = X[query] if form != 'vectors' else query.astype(dt)
    n, V, lse = len(Q), len(X), None
    if form == 'predict':
        S = Q @ params[2].astype(dt).T + params[3].astype(dt)
        lse = S.max(1) + np.log(np.exp(S - S.max(1)[:, None]).sum(1))
    else:
        S = Q @ X.T
        if metric == 'cosine':
            norms = [np.sqrt((A * A).sum(1)) for A in (Q, X)]
            r = [np.divide(1, x, out=np.zeros_like(x), where=x > 0) for x in norms]   # (0 for the zero vector)
            S = S * r[0][:, None] * r[1][None, :]
        if form == 'ids':
            S[np.arange(n), query] = -np.inf
    order = np.lexsort((np.broadcast_to(np.arange(V), S.shape), -S))
    vals = np.take_along_axis(S, order, 1)
    ids = np.where(np.isinf(vals), -1, order)
    pad = max(k - V, 0)
    ids = np.pad(ids, ((0, 0), (0, pad)), constant_values=-1)[:, :k]
    vals = np.pad(vals, ((0, 0), (0, pad)), constant_values=-np.inf)[:, :k]
    if form == 'predict':
        S, vals = np.exp(S - lse[:, None]), np.exp(vals - lse[:, None])
    return ids, vals, lse, S


def make_case(V, E, n, pattern):
    """Parameters, query ids and query rows.  'float': uniform draws with one zero row X_z planted and asked for;
    otherwise integers: 'ascending' has scores ascending with id (every tile overturns the lists), 'first' / 'last'
    put the best keys only in the first / last tile."""
    rng = np.random.default_rng(1000 * V + E)
    ids = rng.integers(0, V, n).astype(np.int32)   # (repeated ids)
    ids[0], ids[-1] = V - 1, 0
    if pattern == 'float':
        a, z = np.sqrt(3.0 / E), V // 2
        Ein, Eout = rng.uniform(-a, a, (V, E)), rng.uniform(-a, a, (V, E))
        b1, b2 = rng.uniform(-0.1, 0.1, E), rng.uniform(-1, 1, V)
        Ein[z] = -b1
        q = rng.uniform(-1, 1, (n, E))
        if n > 1:
            ids[1], q[1] = z, 0
    else:
        Ein, b1 = rng.integers(-2, 3, (V, E)), rng.integers(-1, 2, E)
        Eout, b2 = rng.integers(-1, 2, (V, E)), rng.integers(-3, 4, V)
        q = rng.integers(-2, 3, (n, E))
        q[0] = 1
        if pattern == 'ascending':
            Ein[:], b1[:], Eout[:], b2 = (5 * np.arange(V) // V - 2)[:, None], 0, 0, np.arange(V) // 3
        elif pattern != 'random':
            best = slice(0, 5) if pattern == 'first' else slice(-5, None)
            Ein, b1[:] = np.minimum(Ein, 1), 1
            Ein[best] = 2
            b2[best] += 20
    return [x.astype(np.float32) for x in (Ein, b1, Eout, b2)], ids, q.astype(np.float32)


def ask(m, form, ids, q, k, metric):
    if form == 'predict':
        return m.predict(ids, k)
    return m.neighbors(ids, k, metric) if form == 'ids' else m.neighbors_vectors(q, k, metric)


def check_splits(m, V, n):
    """Both merge paths without a hook: the one-query case runs with several splits, the widest batch with one."""
    if n == 1 and V > 32:
        assert m.query_stats()['splits'] > 1
    if n == ONE_SPLIT_N:
        assert m.query_stats()['splits'] == 1


@pytest.mark.parametrize('pattern', ['random', 'ascending', 'first', 'last'])
@pytest.mark.parametrize('V,E,n,k', SHAPES)
def test_exact(V, E, n, k, pattern):
    params, ids, q = make_case(V, E, n, pattern)
    m = pkg.SkipgramModel(0, V, E)
    m.set_params(*params)
    for form in FORMS:
        got = ask(m, form, ids, q, k, 'dot')
        want = rule(params, form, q if form == 'vectors' else ids, 'dot', k)
        assert np.array_equal(got[0], want[0]), (form, got[0][:2], want[0][:2])
        if form != 'predict':
            assert np.array_equal(got[1], want[1]), (form, got[1][:2], want[1][:2])
        if form == 'ids':
            assert not (got[0] == ids[:, None]).any()
        check_splits(m, V, n)
    m.close()


def rel_err(x, x64):
    x64 = np.where(np.isinf(x64), 0, x64)
    den = np.abs(x64).max()
    return float(np.abs(np.where(np.isinf(x), 0, x).astype(np.float64) - x64).max() / (den if den else 1.0))


@pytest.mark.parametrize('V,E,n,k', SHAPES)
def test_float(V, E, n, k):
    params, ids, q = make_case(V, E, n, 'float')
    m = pkg.SkipgramModel(0, V, E)
    m.set_params(*params)
    errs = {'cosine': 0.0, 'prob': 0.0, 'lse': 0.0}
    for form in FORMS:
        kind = 'prob' if form == 'predict' else 'cosine'
        got = ask(m, form, ids, q, k, 'cosine')
        wi, wv, wlse, S = rule(params, form, q if form == 'vectors' else ids, 'cosine', k)
        live = wi >= 0
        assert np.array_equal(got[0] >= 0, live)   # the padding: id -1 with -inf or probability 0
        assert np.array_equal(got[1][~live], np.where(form == 'predict', 0, wv)[~live])
        assert (got[0][live] < V).all() and all(len(set(r[r >= 0])) == (r >= 0).sum() for r in got[0][:200])
        assert form != 'ids' or not (got[0] == ids[:, None]).any()
        scale = np.abs(S[np.isfinite(S)]).max() if np.isfinite(S).any() else 1.0
        at_ids = np.take_along_axis(S, np.maximum(got[0], 0), 1)   # the float64 value at each returned id
        e_ids = np.abs(at_ids[live] - got[1][live]).max(initial=0) / (scale or 1.0)
        e_pos = np.abs(wv[live] - got[1][live]).max(initial=0) / (scale or 1.0)
        errs[kind] = max(errs[kind], e_ids, e_pos)
        if form == 'predict':
            errs['lse'] = rel_err(got[2], wlse)
        else:   # the planted zero vector scores 0 against everything, and everything against it
            assert not got[1][got[0] == V // 2].any() and (n == 1 or not got[1][1][live[1]].any())
        check_splits(m, V, n)
    print(V, E, n, k, errs)
    assert all(errs[kind] <= TOL[kind] for kind in errs), errs
    m.close()


def routes_check():
    import torch
    V, E, n, k = 131, 50, 70, 10
    params, ids, q = make_case(V, E, n, 'float')
    m = pkg.SkipgramModel(0, V, E)
    m.set_params(*params)
    dev = lambda x: torch.from_numpy(x).cuda()
    for host, tensors, arg in ((m.neighbors, m.neighbors_tensors, ids), (m.neighbors_vectors, m.neighbors_vectors_tensors, q),
                               (m.predict, m.predict_tensors, ids)):
        a, b, c = host(arg, k), host(arg, k), tensors(dev(arg), k)
        assert all(x.tobytes() == y.tobytes() == z.cpu().numpy().tobytes() for x, y, z in zip(a, b, c))
    # the id form is the vector form of the embedded rows with the query itself taken out
    for metric in ('dot', 'cosine'):
        gi, gs = m.neighbors(ids, k, metric)
        vi, vs = m.neighbors_vectors(m.embed(ids), k + 1, metric)
        for r in range(n):
            keep = vi[r] != ids[r]
            assert gi[r].tobytes() == vi[r][keep][:k].tobytes() and gs[r].tobytes() == vs[r][keep][:k].tobytes()
    # errors: the message and the code, nothing written, the parameters unchanged
    bad = ids.copy()
    bad[5], bad[9] = V, -1
    for call in (lambda: m.neighbors(bad, k), lambda: m.predict(bad, k), lambda: m.neighbors_tensors(dev(bad), k),
                 lambda: m.predict_tensors(dev(bad), k)):
        with pytest.raises(pkg.BpeError, match=r'skip-gram model id 131 outside \[0, 131\) \(element 5\)') as e:
            call()
        assert e.value.code == pkg.ERR_ARG
    for call, msg in ((lambda: m.neighbors(ids, 0), r'k 0 outside \[1, 64\]'), (lambda: m.predict(ids, 65), r'k 65 outside \[1, 64\]'),
                      (lambda: m.neighbors(ids, k, 'manhattan'), 'metric -1 is neither'),
                      (lambda: m.neighbors_vectors(q[:, :E - 1], k), 'queries of width 49 given to a model of width 50')):
        with pytest.raises(pkg.BpeError, match=msg) as e:
            call()
        assert e.value.code == pkg.ERR_ARG
    oi, ov, ol = torch.full((n, k), 7, dtype=torch.int32).cuda(), torch.full((n, k), 7.0).cuda(), torch.full((n,), 7.0).cuda()
    torch.cuda.synchronize()
    lib, d_bad = pkg.lib(), dev(bad)
    assert lib.bpe_sgmodel_neighbors_device(m._m, d_bad.data_ptr(), n, k, pkg.SGM_COSINE, oi.data_ptr(), ov.data_ptr()) == pkg.ERR_ARG
    assert lib.bpe_sgmodel_predict_device(m._m, d_bad.data_ptr(), n, k, oi.data_ptr(), ov.data_ptr(), ol.data_ptr()) == pkg.ERR_ARG
    assert (oi == 7).all() and (ov == 7).all() and (ol == 7).all()
    assert m.neighbors([], k)[0].shape == (0, k)
    assert all(np.array_equal(a, b) for a, b in zip(m.get_params(), params))
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


if __name__ == '__main__' and sys.argv[1:] == ['routes']:
    import torch  # noqa: F401  (before libbpe loads)
    print('routes ok' if routes_check() else 'failed')
