"""Two ranks sharing the GPU (gloo collectives on host copies): GpuShard + the export / select /
tie-position C ABI + the exchange protocol, against a single engine on the whole corpus."""
import os
import socket

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def worker(rank, world, port, q, mode='step', n=60, max_length=0, seed=777, A=40, base=60,
           mib=3, corpus='uniform', backend='gloo', engine_mode='stream', rank_loop='native',
           env=None, views=False):
    import importlib
    import sys
    os.environ['BPE_RANK_LOOP'] = rank_loop
    os.environ.update(env or {})
    import torch
    import torch.distributed as dist
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    sharded = importlib.import_module('bpe-tokenizer_amd.sharded')
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    torch.cuda.set_device(0)
    if backend == 'nccl':     # (RCCL: one rank per device, so world 1 on the one-GPU box)
        dist.init_process_group('nccl', rank=rank, world_size=world,
                                device_id=torch.device('cuda', 0))
    else:
        dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        tr = sharded.ShardedTrainer.synthetic(device=0, rank=rank, world=world,
                                              bytes_per_rank=mib << 20, sample_bytes=1 << 20,
                                              seed=seed, alphabet=A, base=base, dist=dist,
                                              corpus=corpus, rank_loop=True)
        assert tr.exchange and dist.get_backend() == backend
        native = rank_loop == 'native' and backend == 'nccl'
        if engine_mode != 'stream':   # ('stream_explicit': the stream, chosen by the caller)
            tr.set_mode('stream' if engine_mode == 'stream_explicit' else engine_mode)
        tr.engine.stats_enable(True)
        if mode == 'step':
            for _ in range(n):
                if tr.step(max_length, 2) is None:
                    break
        else:
            tr.run(n, max_length, 2)     # the device-resident rank loop
        # (views: this rank's copy of the global tables and its exchange buffer, before anything
        # reads the corpus: test_global_state.check_global in the parent)
        view = (tr.engine.maintained_tables(), tr.engine.global_state()) if views else None
        ids, off = tr.engine.read_corpus()
        if mode != 'step':
            assert tr._native == native, (tr._native, native)   # (the path asked for ran)
        st = dict(tr.engine.stats(), trainer_pix_fallbacks=tr.pix_fallbacks)
        q.put((rank, tr.merges, ids.tolist(), off.tolist(), st, view))
    finally:
        dist.destroy_process_group()


def run_ranks(world, **kw):
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=worker, args=(r, world, port, q), kwargs=kw) for r in range(world)]
    for p in procs:
        p.start()
    res = dict((r, rest) for r, *rest in (q.get(timeout=300) for _ in procs))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return res


def single_engine(world, n=60, max_length=0, seed=777, A=40, base=60, mib=3, corpus='uniform', **_):
    # (the reference result: one context, the streaming mode)
    from bpe_amd import pkg
    if corpus == 'zipf':
        data = pkg.synth_zipf((mib * world) << 20, seed=seed, sample_bytes=1 << 20)
    else:
        data = pkg.synth_latin1((mib * world) << 20, seed=seed, A=A, base=base)
    e = pkg.Engine(0)
    e.add_latin1(data, sample_bytes=1 << 20)
    want = e.merge_until(max_length, 2, n)
    ids, off = e.read_corpus()
    tokens = e.num_tokens()
    e.close()
    return want, ids.tolist(), off, tokens


def check(world, **kw):
    res = run_ranks(world, **kw)
    want, ids, off, tokens = single_engine(world, **kw)
    for r in range(world):
        assert [tuple(m) for m in res[r][0]] == want, 'rank %d merges' % r
    assert sum((res[r][1] for r in range(world)), []) == ids
    if kw.get('views'):
        # every rank's copy of the global state against a recount of the single engine's corpus
        from test_global_state import check_global
        from test_maintained_state import pair_count_arrays
        views = [dict(zip(('hot', 'keys', 'counts'), res[r][4][0]), state=res[r][4][1][0], xchg=res[r][4][1][1])
                 for r in range(world)]
        assert all(v['state']['held'] and v['state']['pending'] for v in views), [v['state'] for v in views]
        a, b, W = want[-1]
        check_global(views, *pair_count_arrays(np.array(ids), off), (a, b, tokens - 1, W))
    return [res[r][3] for r in range(world)]


def test_two_ranks_on_one_gpu_match_single_engine():
    check(2)


def test_rank_loop_two_ranks_match_single_engine():
    """The device-resident exchange (bpe_rank_loop_*): 300 merges, past the 256 base ids (cold
    sketch pairs, heavy-bucket iterations through the host protocol) and many tied iterations
    (full tie pass per shard, all-reduce(MAX) of the positions)."""
    check(2, mode='loop', n=300)


def test_rank_loop_three_ranks_max_length():
    check(3, mode='loop', n=200, max_length=3, seed=4242, A=12, base=97, mib=2)


def test_rank_loop_maintained_state_on_zipf_words():
    """A skewed corpus (Zipf words): the cold pairs outgrow the sketch, so the ranks move to the
    maintained state (every rank holds the global tables; each merge exchanges only the delta
    rows of the pairs it touched, bpe_set_global_counts) and stay there: most merges in that
    state, few host iterations, the same merges and corpus as one engine; and at the end the two
    ranks' tables and pending delta rows equal a recount of that corpus
    (test_global_state.check_global)."""
    st = check(2, mode='loop', n=700, corpus='zipf', mib=4, seed=12345, views=True)
    for s in st:
        assert s['fused_passes'] > 300, s
        assert s['loop_host'] <= 12, s


def test_rank_loop_maintained_state_three_ranks_max_length():
    st = check(3, mode='loop', n=400, corpus='zipf', mib=2, seed=99, max_length=6)
    assert all(s['fused_passes'] > 100 for s in st), st


# ---- the RCCL leg (torch.distributed 'nccl' = RCCL on ROCm), one rank on the one-GPU box ----------
# ShardedTrainer(rank_loop=True) runs the N-rank protocol at world 1: the per-iteration
# all-reduce(SUM) of the exchange buffer and all-reduce(MAX) of the tie words go through RCCL on the
# engine's stream, exactly as on 8 GPUs (core.ts:265-267 shards at samples).

@pytest.mark.parametrize('impl', ['native', 'python'])
def test_rccl_rank_loop_one_rank_c3_slice(impl):
    """64 MiB of the C3 stream (256-char alphabet), 400 merges through the rank loop over a 1-rank
    RCCL group: the same merges and corpus as the single-context device loop.  native: the
    all-reduces issued from C++ on the engine's own communicator (bpe_rank_loop_rccl); python:
    torch.distributed calls per iteration."""
    st = check(1, mode='loop', n=400, seed=12345, A=256, base=0, mib=64, backend='nccl',
               rank_loop=impl)
    assert st[0]['tie_passes'] + st[0]['tie_tail'] > 0 or st[0]['iterations'] >= 400, st


def test_rccl_rank_loop_one_rank_zipf_maintained():
    """Zipf words (skewed): the rank moves to the maintained state (global tables kept with delta
    rows, exchanged through RCCL every merge) and stays there."""
    st = check(1, mode='loop', n=600, corpus='zipf', mib=8, seed=12345, backend='nccl')
    assert st[0]['fused_passes'] > 300, st
    assert st[0]['loop_host'] <= 12, st


def test_rccl_host_protocol_one_rank():
    """The host protocol (exchange_and_select: table all-reduce, heavy-bucket all-gathers, tie
    all-reduce) over a 1-rank RCCL group, iteration by iteration."""
    check(1, mode='step', n=120, seed=4242, A=12, base=97, mib=2, backend='nccl')


# ---- the incremental mode over ranks: every rank's position index holds its own lists and the
# global counts; each merge's count changes cross as signed delta rows in the rank loop's
# all-reduce(SUM), R3 ties as the ranks' last counted occurrences in the all-reduce(MAX) ---------

def test_incremental_rank_loop_two_ranks():
    st = check(2, mode='loop', n=300, seed=12345, A=256, base=0, mib=4, engine_mode='incremental')
    assert all(s['pix_merges'] >= 250 for s in st), st


def test_incremental_rank_loop_three_ranks_zipf_max_length():
    st = check(3, mode='loop', n=400, corpus='zipf', mib=2, seed=99, max_length=6,
               engine_mode='incremental')
    assert all(s['pix_merges'] >= 300 for s in st), st


def test_rccl_incremental_rank_loop_one_rank():
    """The incremental mode's rank loop over a 1-rank RCCL group (the delta rows and tie words
    through RCCL on the engine's stream): the same merges and corpus as one context."""
    st = check(1, mode='loop', n=500, corpus='zipf', mib=8, seed=12345, backend='nccl',
               engine_mode='incremental')
    assert st[0]['pix_merges'] >= 400, st


def test_incremental_rank_loop_automatic_switch_and_fallback():
    """The streaming rank loop's switch to the incremental mode past a vocabulary size (18432
    ids; BPE_AUTO_PIX_VOCAB=400 here), and, when an index build fails on some rank
    (BPE_PIX_FORCE_OOM=1, as out of device memory), every rank's agreed fall-back to the stream:
    the same merges and corpus as one context either way.  A mode the caller set
    (set_mode('stream')) is kept: no switch."""
    st = check(2, mode='loop', n=300, seed=12345, A=256, base=0, mib=2,
               env={'BPE_AUTO_PIX_VOCAB': '400'})
    assert all(s['pix_merges'] >= 100 and s['trainer_pix_fallbacks'] == 0 for s in st), st
    st = check(2, mode='loop', n=300, seed=12345, A=256, base=0, mib=2,
               env={'BPE_AUTO_PIX_VOCAB': '400', 'BPE_PIX_FORCE_OOM': '1'})
    assert all(s['pix_merges'] == 0 and s['trainer_pix_fallbacks'] >= 1 for s in st), st
    st = check(2, mode='loop', n=300, seed=12345, A=256, base=0, mib=2,
               env={'BPE_AUTO_PIX_VOCAB': '400'}, engine_mode='stream_explicit')
    assert all(s['pix_merges'] == 0 and s['trainer_pix_fallbacks'] == 0 for s in st), st
