"""One-rank-per-GPU driver of the merge loop (mergeUntil, core.ts:365-383) over a corpus sharded
at sample boundaries.

Pairs never cross samples (core.ts:265-267), so rank r owns a contiguous run of whole samples and
counts its pairs locally (libbpe's streaming pass).  Per iteration the ranks exchange:
  1. the pair table (81920 x u64: exact counts of the pairs of ids < 256 + a count sketch of
     every other pair): one all-reduce(SUM) over RCCL/xGMI;
  2. only when a sketch bucket could still reach the best hot count (every rank decides this
     alike from the global table, so otherwise no collective runs): every rank counts those cold
     pairs exactly (one more streaming pass), then an all-gather of the (key, count) lists with
     duplicates summed on device;
  3. only when several pairs tie on (W, a+b): an all-reduce(MAX) of their last counted positions
     (rule R3; rank r's positions order after rank r-1's).
Every rank then selects the same merge (libbpe's argmax over the global tables) and applies it to
its own shard.  world == 1 is the plain single-GPU loop, unless the trainer is made with
rank_loop=True: then one rank runs the same exchange protocol and rank loop as N ranks (its
collectives over a 1-rank process group), which is how the RCCL leg is exercised on a one-GPU box.

ShardedTrainer.run() keeps that exchange on the device (libbpe's rank loop, include/bpe.h
bpe_rank_loop_*): per iteration the table all-reduce(SUM), the selection kernels, the tie
all-reduce(MAX), the decision and the fused apply+count pass are enqueued in order on the
engine's HIP stream, with no host sync until the end of a batch of BPE_LOOP_BATCH iterations.
Only an iteration with heavy sketch buckets or too many tied pairs takes the host protocol above.
When two host iterations in a row needed exact cold counts (skewed corpora, large vocabularies),
the ranks move to the maintained state: every rank holds the global hot and cold tables (the
all-reduced table + every rank's exact cold-pair list, all-gathered), and each iteration exchanges
only the delta rows of the pairs the merge touched (bpe_set_global_counts, include/bpe.h).

The protocol only needs a `shard` object with export()/select()/tie_positions()/apply(); GpuShard
wraps libbpe on a HIP device, and tests/test_sharded_gloo.py drives the same protocol on CPU
with gloo.
"""
import importlib
import os

import numpy as np

pkg = importlib.import_module('bpe-tokenizer_amd')

HOT_BINS = 256 * 256
TABLE_BINS = HOT_BINS + 16384
MAX_CAND = 16            # BPE_MAX_CAND: tie positions all-reduced per iteration
LOOP_BATCH = 64          # BPE_LOOP_BATCH: iterations per host round trip of the rank loop
AUTO_PIX_VOCAB = 18432   # the streaming mode goes on in the incremental mode here (bpe_multi.cpp)
RANK_SHIFT = 40          # global position = rank << 40 | shard-local position


def first_appearance(data, alphabet_size=256):
    """Position of the first occurrence of every byte value (-1 if absent).  Scans in blocks and
    stops once `alphabet_size` distinct values have been seen."""
    first = np.full(256, -1, np.int64)
    seen = 0
    step = 1 << 16
    for s in range(0, len(data), step):
        u, idx = np.unique(data[s:s + step], return_index=True)
        new = first[u] < 0
        first[u[new]] = idx[new] + s
        seen += int(new.sum())
        if seen >= alphabet_size:
            break
    return first


def hip_runtimes():
    """The distinct libamdhip64 files mapped into this process.  PyTorch's wheel bundles its own
    (same soname as /opt/rocm/lib's): imported BEFORE libbpe is loaded, libbpe binds to it and the
    process has one HIP runtime; loaded after libbpe, the process holds two, and device pointers
    and streams of one are not valid in the other."""
    try:
        with open('/proc/self/maps') as f:
            return sorted({l.split()[-1] for l in f if 'libamdhip64' in l and '/' in l})
    except OSError:
        return []


class GpuShard:
    """libbpe engine on one HIP device, exporting/selecting through torch device tensors."""

    def __init__(self, engine, device_index):
        import torch
        rt = hip_runtimes()
        if len(rt) > 1:
            raise RuntimeError('libbpe and torch run on different HIP runtimes (%s): import torch '
                               'before the first libbpe call in a process that shares device '
                               'buffers between them' % ', '.join(rt))
        self.engine = engine
        self.torch = torch
        self.device = torch.device('cuda', device_index)
        self.table = torch.zeros(TABLE_BINS, dtype=torch.int64, device=self.device)
        self.cap = 1 << 16
        self.keys = torch.zeros(self.cap, dtype=torch.int32, device=self.device)
        self.counts = torch.zeros(self.cap, dtype=torch.int64, device=self.device)

    def export(self):
        self.engine.export_counts(self.table.data_ptr())
        return self.table

    def heavy(self, table, max_length):
        torch = self.torch
        table = table.contiguous()
        n = self.engine.heavy_counts(table.data_ptr(), self.keys.data_ptr(), self.counts.data_ptr(),
                                     self.cap, max_length)
        if n < 0:
            return None   # no heavy bucket anywhere (same decision on every rank)
        for _ in range(3):
            # (n counts the claims that lost a race too: the pass again may list a few more)
            if n <= self.cap:
                break
            self.cap = 1 << max(16, int(n + n // 8).bit_length())
            self.keys = torch.zeros(self.cap, dtype=torch.int32, device=self.device)
            self.counts = torch.zeros(self.cap, dtype=torch.int64, device=self.device)
            n = self.engine.heavy_counts(table.data_ptr(), self.keys.data_ptr(),
                                         self.counts.data_ptr(), self.cap, max_length)
        if n > self.cap:
            raise RuntimeError('bpe sharded: the heavy cold list (%d) outgrew its buffers (%d) three times'
                               % (n, self.cap))
        return self.keys[:n], self.counts[:n]

    def select(self, table, keys, counts, max_length, min_weight):
        table = table.contiguous()
        keys = keys.contiguous()
        counts = counts.contiguous()
        return self.engine.select_counts(table.data_ptr(), keys.data_ptr() if keys.numel() else None,
                                         counts.data_ptr() if counts.numel() else None,
                                         keys.numel(), max_length, min_weight)

    def tie_positions(self, cands):
        return self.engine.tie_positions(cands)

    def apply(self, a, b, c):
        return self.engine.apply_merge(a, b, c, sync=False)


def exchange_and_select(shard, dist, rank, world, max_length=0, min_weight=0, info=None):
    """The per-iteration collective protocol.  Returns (a, b, W) or None, identical on every rank.
    Collectives run on the tables' device (RCCL); with the gloo backend on host copies.
    info (a dict): receives 'heavy', whether exact cold counts were needed."""
    import torch
    table = shard.export()
    dev = torch.device('cpu') if dist.get_backend() == 'gloo' else table.device
    sdev = getattr(shard, 'device', dev)
    table = table.to(dev, copy=True)
    dist.all_reduce(table)
    gtable = table.to(sdev)

    def sync():
        # (collectives and copies run on torch's stream, the engine reads on its own)
        if getattr(gtable, 'is_cuda', False):
            torch.cuda.synchronize(gtable.device)
    sync()
    heavy = shard.heavy(gtable, max_length)                  # identical decision on every rank
    if info is not None:
        info['heavy'] = heavy is not None
    m = 0
    if heavy is not None:
        keys, counts = heavy
        keys = keys.to(dev)
        counts = counts.to(dev)
        n = torch.tensor([keys.numel()], dtype=torch.int64, device=dev)
        sizes = [torch.zeros_like(n) for _ in range(world)]
        dist.all_gather(sizes, n)
        sizes = [int(x.item()) for x in sizes]
        m = max(sizes)
    if m:
        kp = torch.full((m,), -1, dtype=torch.int32, device=dev)
        cp = torch.zeros(m, dtype=torch.int64, device=dev)
        kp[:keys.numel()] = keys
        cp[:counts.numel()] = counts
        gk = [torch.empty_like(kp) for _ in range(world)]
        gc = [torch.empty_like(cp) for _ in range(world)]
        dist.all_gather(gk, kp)
        dist.all_gather(gc, cp)
        all_k = torch.cat([g[:s] for g, s in zip(gk, sizes)])
        all_c = torch.cat([g[:s] for g, s in zip(gc, sizes)])
        ukeys, inv = torch.unique(all_k, return_inverse=True)
        ucounts = torch.zeros(ukeys.numel(), dtype=torch.int64, device=dev).index_add_(0, inv, all_c)
    else:
        ukeys = torch.zeros(0, dtype=torch.int32, device=dev)
        ucounts = torch.zeros(0, dtype=torch.int64, device=dev)
    ukeys, ucounts = ukeys.to(sdev), ucounts.to(sdev)
    sync()
    sel = shard.select(gtable, ukeys, ucounts, max_length, min_weight)
    if sel is None:
        return None
    w, cands = sel
    a, b = cands[0]
    if len(cands) > 1:
        last = np.asarray(shard.tie_positions(cands), dtype=np.int64)
        glob = np.where(last > 0, (np.int64(rank) << RANK_SHIFT) | last, 0)
        g = torch.tensor(glob, dtype=torch.int64, device=dev)
        dist.all_reduce(g, op=dist.ReduceOp.MAX)
        g = g.cpu().numpy()
        best = None
        for (ca, cb), pos in zip(cands, g):
            if pos > 0 and (best is None or pos < best[0]):
                best = (pos, ca, cb)
        a, b = best[1], best[2]
    return a, b, w


class ShardedTrainer:
    def __init__(self, shard, rank, world, dist, n_tokens, live_global, rank_loop=False):
        self.shard = shard
        # the exchange protocol and the rank loop (always for world > 1; for world 1 on request)
        self.exchange = world > 1 or rank_loop
        self.engine = getattr(shard, 'engine', shard)
        self.rank = rank
        self.world = world
        self.dist = dist
        self.n_tokens = n_tokens          # token_table.length (next new id, core.ts:315)
        self.live = live_global           # live corpus tokens over all ranks
        self.merges = []
        self._rl = None                   # rank loop buffers (exchange, tie, stream)
        # the maintained state (every rank holds the global tables: bpe_set_global_counts), and the
        # host iterations in a row that needed exact cold counts (two: enter that state)
        self._maintained = False
        self._heavy_streak = 0
        # the incremental mode: the global state lives in every rank's position index (entered at
        # once, the tables' counts exchanged as signed delta rows: bpe_pix.hip.h).  As in
        # bpe_multi.cpp: every re-entry builds the index again, so a run whose batches keep handing
        # over (more than 64 entries since set_mode, at least one per 16 merges) goes on in the
        # streaming mode (_pix_off), on every rank alike (the entries and merges are global facts)
        self.pix = False
        self._pix_off = False
        self._pix_entries = self._pix_merged = 0
        # (the incremental mode came from the automatic switch; times its indexes did not fit and
        # the stream went on)
        self._pix_auto = False
        self.pix_fallbacks = 0
        # the caller chose a mode (set_mode): the automatic switch past AUTO_PIX_VOCAB ids leaves it
        self._mode_explicit = False
        # RCCL backend: the rank loop's two all-reduces per iteration are issued from C++ on the
        # engine's stream (bpe_rank_loop_rccl, one call per batch); BPE_RANK_LOOP=python keeps them
        # as torch.distributed calls (A/B)
        self._native = None

    def set_mode(self, mode):
        """'stream' or 'incremental' (bpe_set_mode) for this rank's engine; every rank alike.
        The choice is kept: no automatic switch to the incremental mode follows."""
        self._set_mode(mode)
        self._mode_explicit = True

    def _set_mode(self, mode):
        self.engine.set_mode(mode)
        self.pix = mode == 'incremental'
        self._pix_off = False
        self._pix_auto = False
        self._pix_entries = self._pix_merged = 0
        self._maintained = False

    @classmethod
    def synthetic(cls, device, rank, world, bytes_per_rank, sample_bytes, seed, alphabet, base,
                  dist=None, corpus='uniform', rank_loop=False):
        """Rank r holds bytes [r*B, (r+1)*B) of one synthetic corpus: the
        xorshift32 byte stream ('uniform') or Zipf(1.1) words ('zipf', bpe_synth_zipf; whole
        samples per rank)."""
        if corpus == 'zipf':
            if bytes_per_rank % sample_bytes:
                raise ValueError('zipf shards hold whole samples')
            data = pkg.synth_zipf(bytes_per_rank, seed=seed, sample_bytes=sample_bytes,
                                  first_sample=rank * (bytes_per_rank // sample_bytes))
        else:
            data = pkg.synth_latin1(bytes_per_rank, seed=seed, A=alphabet, base=base,
                                    skip=rank * bytes_per_rank)
        eng = pkg.Engine(device)
        if world == 1 and not rank_loop:
            cmap, nt, _ = eng.add_latin1(data, sample_bytes=sample_bytes)
            return cls(eng, rank, world, dist, nt, bytes_per_rank)
        # global first-appearance order (core.ts:186-199) across the shards, in corpus order
        import torch
        # (the zipf generator's bytes are not the uniform stream's alphabet: look for all 256)
        first = first_appearance(data, 256 if corpus == 'zipf' else alphabet)
        big = np.iinfo(np.int64).max
        key = np.where(first >= 0, (np.int64(rank) << RANK_SHIFT) + first, big)
        t = torch.tensor(key, dtype=torch.int64, device=torch.device('cuda', device))
        dist.all_reduce(t, op=dist.ReduceOp.MIN)
        gkey = t.cpu().numpy()
        order = [int(ch) for ch in np.argsort(gkey, kind='stable') if gkey[ch] != big]
        cmap = np.full(256, -1, np.int32)
        for i, ch in enumerate(order):
            cmap[ch] = i
        for i in range(len(order)):
            eng.set_token_len16(i, 1)
        eng.add_latin1(data, sample_bytes=sample_bytes, char_to_id=cmap, n_tokens=len(order))
        return cls(GpuShard(eng, device), rank, world, dist, len(order), bytes_per_rank * world,
                   rank_loop=rank_loop)

    def live_tokens_global(self):
        return self.live

    def find_next_merge(self, max_length=0, min_weight=0):
        if not self.exchange:
            return self.engine.find_next_merge(max_length, min_weight)
        return exchange_and_select(self.shard, self.dist, self.rank, self.world, max_length,
                                   min_weight)

    def run(self, n, max_length=0, min_weight=0):
        """n merge iterations (fewer when no pair qualifies); returns the merges [(a, b, W)].
        On one GPU this is the engine's mergeUntil (decisions stay on the device, one host sync
        per batch of iterations); across ranks every iteration exchanges counts (step())."""
        if not self.exchange:
            ms = self.engine.merge_until(max_length, min_weight, n)
            for m in ms:
                self.n_tokens += 1
                self.live -= m[2]
            self.merges += ms
            return ms
        return self.run_rank_loop(n, max_length, min_weight)

    def _collectives(self):
        dist = self.dist
        gloo = dist.get_backend() == 'gloo'

        def all_reduce(t, op):
            if gloo:           # (host copies, in order on the engine's stream; tests only)
                h = t.cpu()
                dist.all_reduce(h, op=op)
                t.copy_(h)
            else:              # RCCL, ordered after the stream's kernels by events
                dist.all_reduce(t, op=op)
        return gloo, all_reduce

    def _check_same_exchange(self, nw, gloo):
        """Every rank must all-reduce the same number of words this batch (a rank whose tables
        left the global state would exchange a different buffer): checked as bpe_multi.cpp does,
        by an all-reduce(MAX) of (nw, -nw) once per batch."""
        import torch
        dev = torch.device('cpu') if gloo else self.shard.device
        t = torch.tensor([nw, -nw], dtype=torch.int64, device=dev)
        self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX)
        hi, lo = int(t[0].item()), -int(t[1].item())
        if hi != nw or lo != nw:
            raise RuntimeError('bpe sharded: ranks disagree on the exchange (%d words here, %d..%d '
                               'over the ranks)' % (nw, lo, hi))

    def enter_maintained(self):
        """The maintained state over the ranks (skewed corpora, large vocabularies): the global
        table, and every rank's exact cold-pair list all-gathered, become every rank's global
        tables (bpe_cold_counts / bpe_set_global_counts); the rank loop then keeps them with
        delta rows instead of exchanging whole tables."""
        import torch
        dist, eng = self.dist, self.engine
        gloo, all_reduce = self._collectives()
        dev = self.shard.device
        # (torch's work here runs on its own stream: synchronized before each engine call that
        # reads or writes a tensor made there, which the engine's stream would otherwise race)
        table = self.shard.export().clone()
        all_reduce(table, dist.ReduceOp.SUM)
        n = eng.cold_counts(None, None, 0)                     # (the pass; kept for the export)
        cap = max(1, n)
        keys = torch.full((cap,), -1, dtype=torch.int32, device=dev)
        counts = torch.zeros(cap, dtype=torch.int64, device=dev)
        torch.cuda.synchronize(dev)
        eng.cold_counts(keys.data_ptr(), counts.data_ptr(), cap)
        cdev = torch.device('cpu') if gloo else dev
        size = torch.tensor([n], dtype=torch.int64, device=cdev)
        sizes = [torch.zeros_like(size) for _ in range(self.world)]
        dist.all_gather(sizes, size)
        sizes = [int(x.item()) for x in sizes]
        m = max(1, max(sizes))
        kp = torch.full((m,), -1, dtype=torch.int32, device=cdev)
        cp = torch.zeros(m, dtype=torch.int64, device=cdev)
        kp[:n] = keys[:n].to(cdev)
        cp[:n] = counts[:n].to(cdev)
        gk = [torch.empty_like(kp) for _ in range(self.world)]
        gc = [torch.empty_like(cp) for _ in range(self.world)]
        dist.all_gather(gk, kp)
        dist.all_gather(gc, cp)
        all_k = torch.cat([g[:z] for g, z in zip(gk, sizes)] + [kp[:0]]).to(dev).contiguous()
        all_c = torch.cat([g[:z] for g, z in zip(gc, sizes)] + [cp[:0]]).to(dev).contiguous()
        total = all_k.numel()
        torch.cuda.synchronize(dev)
        pix = self.pix and not self._pix_off
        try:
            eng.set_global_counts(table.data_ptr(), all_k.data_ptr() if total else None,
                                  all_c.data_ptr() if total else None, total)
            ok = 1
        except pkg.BpeError as e:
            # (only "the index does not fit" (BPE_ERR_NOFIT) after the automatic switch: any
            # other error, a HIP fault or a table overflow, is the caller's)
            if not (pix and self._pix_auto and e.code == pkg.ERR_NOFIT):
                raise
            ok = 0      # (this rank's index does not fit beside its corpus)
        if pix and self._pix_auto:
            # every rank alike: after the automatic switch, an index that does not fit on some
            # rank sends every rank back to the stream (as bpe_multi.cpp)
            flag = torch.tensor([ok], dtype=torch.int32, device=cdev)
            dist.all_reduce(flag, op=dist.ReduceOp.MIN)
            if int(flag.item()) == 0:
                self._pix_off = True
                self.pix_fallbacks += 1
                eng.set_mode('stream')
                return self.enter_maintained()
        self._maintained = True
        self._heavy_streak = 0

    def _native_rccl(self, gloo):
        """The engine's own RCCL communicator for the rank loop (bpe_rank_rccl_init), made once: rank 0's
        unique id broadcast over the process group."""
        if self._native is None:
            self._native = False
            if not gloo and os.environ.get('BPE_RANK_LOOP', 'native') != 'python':
                import torch
                uid = torch.zeros(128, dtype=torch.uint8, device=self.shard.device)
                if self.rank == 0:
                    uid.copy_(torch.frombuffer(bytearray(pkg.rccl_unique_id()), dtype=torch.uint8))
                self.dist.broadcast(uid, src=0)
                self.engine.rccl_init(bytes(uid.cpu().numpy().tobytes()), self.rank, self.world)
                self._native = True
        return self._native

    def run_rank_loop(self, n, max_length=0, min_weight=0):
        """n iterations across the ranks with the exchange on the device (bpe_rank_loop_*): no
        host sync inside a batch of LOOP_BATCH iterations.  Returns the merges [(a, b, W)]."""
        import torch
        dist = self.dist
        eng = self.engine
        if self._rl is None:
            dev = self.shard.device
            # (poisoned: the rank loop must not rely on the buffers' contents, include/bpe.h)
            self._rl = (torch.full((pkg.XCHG_WORDS,), -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device=dev),
                        torch.full((pkg.TIE_WORDS,), -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device=dev),
                        torch.cuda.ExternalStream(eng.stream(), device=dev))
        xchg, tie, stream = self._rl
        gloo, all_reduce = self._collectives()
        ms = []
        batch = LOOP_BATCH      # (as bpe_merge_until: about twice what an early-ended batch did)
        while len(ms) < n:
            k = min(batch, n - len(ms))
            # (as bpe_multi.cpp: past AUTO_PIX_VOCAB token ids the streaming mode's maintained state
            # outgrows its LDS rows and its scans of the claimed cold pairs; the ranks go on in the
            # incremental mode, same merges.  A mode the caller set is kept; BPE_STREAM_ONLY=1
            # keeps the stream)
            if (not self.pix and not self._mode_explicit
                    and self.n_tokens >= int(os.environ.get('BPE_AUTO_PIX_VOCAB', AUTO_PIX_VOCAB))
                    and not os.environ.get('BPE_STREAM_ONLY')):
                self._set_mode('incremental')
                self._pix_auto = True
            pix = self.pix and not self._pix_off
            if not self._maintained and (self._heavy_streak >= 2 or pix):
                if pix:
                    self._pix_entries += 1
                    if self._pix_entries > 64 and self._pix_entries > (self._pix_merged + len(ms)) // 16:
                        self._pix_off = True
                        self.engine.set_mode('stream')
                self.enter_maintained()
            batch_maintained = self._maintained
            with torch.cuda.stream(stream):
                nw = eng.rank_loop_begin(max_length, min_weight, xchg.data_ptr(), tie.data_ptr(),
                                         self.rank, self.world)
                self._check_same_exchange(nw, gloo)
                if self._native_rccl(gloo):
                    eng.rank_loop_rccl(xchg.data_ptr(), nw, tie.data_ptr(), k)
                else:
                    view = xchg[:nw]
                    for _ in range(k):
                        all_reduce(view, dist.ReduceOp.SUM)
                        eng.rank_loop_select()
                        all_reduce(tie, dist.ReduceOp.MAX)
                        eng.rank_loop_decide()
                        eng.rank_loop_count()
                got, reps, status = eng.rank_loop_end()
            if got:
                # every merge: the ranks' replacement counts sum to W (core.ts:356-359)
                r = torch.tensor(reps, dtype=torch.int64,
                                 device=torch.device('cpu') if gloo else self.shard.device)
                dist.all_reduce(r)
                if [int(v) for v in r.cpu().tolist()] != [m[2] for m in got]:
                    raise RuntimeError('bpe sharded: replacement counts do not sum to W')
            for m in got:
                self.n_tokens += 1
                self.live -= m[2]
            self.merges += got
            ms += got
            if status != 0:
                self._maintained = False      # (the engines left the global state)
            if status == 1:
                break
            batch = min(LOOP_BATCH, 2 * batch if status == 0 else max(1, 2 * len(got)))
            if status == 2 and len(ms) < n:
                info = {}
                m = self.step(max_length, min_weight, info)     # the host protocol for this iteration
                heavy = info.get('heavy', False)
                self._heavy_streak = (max(self._heavy_streak + 1, 2 if batch_maintained else 1)
                                      if heavy else 0)
                if m is None:
                    break
                ms.append(m)
        if self.pix:
            self._pix_merged += len(ms)
        return ms

    def step(self, max_length=0, min_weight=0, info=None):
        """One findNextMerge + applyMerge on every rank; returns (a, b, W) or None."""
        self._maintained = False
        if not self.exchange:
            m = self.engine.find_next_merge(max_length, min_weight)
        else:
            m = exchange_and_select(self.shard, self.dist, self.rank, self.world, max_length,
                                    min_weight, info)
        if m is None:
            return None
        a, b, w = m
        if not self.exchange:
            self.engine.apply_merge(a, b, self.n_tokens, sync=False)
        else:
            self.shard.apply(a, b, self.n_tokens)   # (no host sync: the count settles lazily)
        self.n_tokens += 1
        self.live -= w
        self.merges.append(m)
        return m
