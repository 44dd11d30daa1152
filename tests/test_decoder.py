"""The device decoder (bpe_decoder_* / bpe_decode_batch, csrc/bpe_decode.hip): decodeVector /
decodeTokens (core.ts:447-471) for batches of texts, checked against

  - the reference's own data (tests/golden/small_cases.json: every vector the reference made
    decodes back to its sample, every token id to its chars), and
  - a ten-line Python decode (join chars[id], vectors mapped through the index first) on seeded
    vocabularies and batches laid out around the kernels' tile size, on both forms (host buffers,
    device tensors), with the engine and the encoder, and on every error the header names.
"""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from bpe_amd import pkg
from golden_util import char_weights, compact_index, load_small, token_table_after
from oracle import Corpus

T = pkg.DECODE_TILE
KINDS = ['ids', 'vectors']


# ---- the Python decode the device is checked against ---------------------------------------------

def units_of(s):
    return np.frombuffer(s.encode('utf-16-le', 'surrogatepass'), dtype='<u2').astype(np.uint16)


def py_decode(texts, chars, index=None):
    """decodeTokens (index None) / decodeVector: join chars[id]."""
    out = []
    for t in texts:
        ids = [int(v) if index is None else int(index[int(v)]) for v in t]
        out.append(''.join(chars[i] for i in ids))
    return out


def py_decode_flat(vals, off, chars, index=None):
    """The same on the flat form: (units uint16, out_off int64)."""
    texts = [vals[off[k]:off[k + 1]] for k in range(len(off) - 1)]
    parts = [units_of(s) for s in py_decode(texts, chars, index)]
    out_off = np.zeros(len(parts) + 1, np.int64)
    np.cumsum([len(p) for p in parts], out=out_off[1:])
    units = np.concatenate(parts) if len(parts) and out_off[-1] else np.zeros(0, np.uint16)
    return units, out_off


def flat(texts, lead=0, junk=-7):
    """texts -> (vals, off) with `lead` values before the first text (off[0] = lead) that no text
    covers: values no table knows, so that reading them would fail the call."""
    off = np.zeros(len(texts) + 1, np.int64)
    np.cumsum([len(t) for t in texts], out=off[1:])
    vals = np.concatenate([np.full(lead, junk, np.int32)] + [np.asarray(t, np.int32) for t in texts])
    return vals.astype(np.int32), off + lead


# ---- 1. the reference's own data --------------------------------------------------------------------

@pytest.mark.gpu
def test_reference_vectors_decode_to_their_samples():
    """Every vector of the 1509 golden cases decodes to the sample it was made from, and every
    token id to the chars of the reference's token table."""
    dec = pkg.Decoder(0)
    n_checked = n_ids = 0
    longest = 0
    try:
        for case in load_small():
            c = Corpus()
            for s in case['samples']:
                c.add(s)
            merges = [tuple(m) for m in case['merges']]
            table = token_table_after(c.chars, char_weights(c.samples, len(c.chars)), merges)
            if not table:
                continue
            dec.clear()
            dec.add_tokens(c.chars)
            if merges:
                dec.add_merges([(a, b, len(c.chars) + k) for k, (a, b, _w) in enumerate(merges)])
            assert dec.num_tokens()[0] == len(table) == len(case['token_table'])
            dec.set_vector_index(list(compact_index(table).keys()))
            pairs = [(v, s) for v, s in zip(case['vectors'], case['samples']) if not isinstance(v, str)]
            got = dec.decode([v for v, _s in pairs], 'vectors')
            for g, (_v, s) in zip(got, pairs):
                assert g == s, case['name']
                n_checked += 1
            got = dec.decode([[i] for i in range(len(table))], 'ids')
            for i, g in enumerate(got):
                assert g == case['token_table'][i][0], (case['name'], i)
                longest = max(longest, len(units_of(g)))
                n_ids += 1
    finally:
        dec.close()
    assert n_checked > 4300, n_checked
    assert n_ids > 4300 and longest == 570, (n_ids, longest)   # (the longest token of the goldens)


# ---- 2. shapes where the kernels can go wrong ---------------------------------------------------------

def edge_vocab():
    """Tokens of 1 unit, of 2 units (surrogate pairs), lone surrogates, an empty-chars token, and a
    doubling chain (c, c) of 13 merges up to 8192 units.  Returns (chars per id, char tokens,
    merges, id of the 8192-unit token)."""
    base = [chr(0x61 + i) for i in range(20)] + ['é', '中', '￿']      # 1 unit
    base += [chr(0x1F600 + i) for i in range(6)] + ['\U0010FFFF']                     # 2 units
    base += ['\ud800', '\udbff', '\udc00', '\udfff']                                  # lone surrogates
    base += ['']                                                                      # no chars
    chars = list(base)
    merges = []
    prev = 0                                                                          # 'a'
    for _ in range(13):
        merges.append((prev, prev, len(chars)))
        chars.append(chars[prev] + chars[prev])
        prev = len(chars) - 1
    # a few ordinary merges after the chain (inputs of every kind)
    for a, b in [(1, 24), (33, 2), (30, 31), (34, 34), (23, 27)]:
        merges.append((a, b, len(chars)))
        chars.append(chars[a] + chars[b])
    assert len(units_of(chars[prev])) == 8192
    return chars, base, merges, prev


def edge_batch(rng, n_small, big):
    """The batch of the issue's list: texts as id lists (ids below n_small only, and `big` where it
    is placed on purpose), with the flat position of every text known."""
    def rand(n):
        return rng.integers(0, n_small, size=n).astype(np.int32)
    texts = [[], [], [1], rand(T - 1), [], rand(T), rand(T + 1), rand(2 * T + 3), [big, big, big]]
    pos = sum(len(t) for t in texts)
    texts.append(rand((T - 1 - pos) % T + T))           # the next text starts one value before a tile edge
    assert sum(len(t) for t in texts) % T == T - 1
    texts += [[big, big, big], rand(7), [], []]
    return texts


def make_edge():
    chars, base, merges, big = edge_vocab()
    rng = np.random.default_rng(5)
    n_small = len(base) + 4                              # chars and the chain up to 16 units
    texts = edge_batch(rng, n_small, big)
    index = rng.permutation(len(chars)).astype(np.int32)   # vector index -> id: every id is live
    inv = np.argsort(index).astype(np.int32)
    return dict(chars=chars, base=base, merges=merges, big=big, texts=texts, index=index, inv=inv)


@pytest.fixture(scope='module')
def edge():
    return make_edge()


def make_decoder(edge):
    dec = pkg.Decoder(0)
    dec.add_tokens(edge['base'])
    dec.add_merges(edge['merges'])
    dec.set_vector_index(edge['index'])
    return dec


def batch_of(edge, kind, lead=5):
    texts = edge['texts'] if kind == 'ids' else [edge['inv'][np.asarray(t, np.int64)] for t in edge['texts']]
    return flat(texts, lead=lead)


@pytest.mark.gpu
@pytest.mark.parametrize('kind', KINDS)
def test_tile_edges_long_tokens_empty_texts(edge, kind):
    dec = make_decoder(edge)
    try:
        assert dec.num_tokens() == (len(edge['chars']), sum(len(units_of(c)) for c in edge['chars']))
        index = None if kind == 'ids' else edge['index']
        for lead in (5, 0):
            vals, off = batch_of(edge, kind, lead)
            assert off[0] == lead
            want, want_off = py_decode_flat(vals, off, edge['chars'], index)
            got, got_off = dec.decode_flat(vals, off, kind)
            assert got.dtype == np.uint16 and np.array_equal(got_off, want_off)
            assert np.array_equal(got, want)
        assert want_off[3] % 2 == 1                       # a text at an odd unit offset
        # no texts at all
        for off0 in ([0], [5]):
            got, got_off = dec.decode_flat(np.zeros(0, np.int32), np.asarray(off0, np.int64), kind)
            assert got.size == 0 and got_off.tolist() == [0]
        # only empty texts
        got, got_off = dec.decode_flat(np.zeros(3, np.int32), np.asarray([3, 3, 3], np.int64), kind)
        assert got.size == 0 and got_off.tolist() == [0, 0, 0]
        # the str form
        texts = [t for t in edge['texts'][:3]] + [edge['texts'][-3]]
        src = texts if kind == 'ids' else [edge['inv'][np.asarray(t, np.int64)] for t in texts]
        assert dec.decode(src, kind) == py_decode(texts, edge['chars'])
    finally:
        dec.close()


# ---- 3. more tiles than one scan round ------------------------------------------------------------------

@pytest.mark.gpu
def test_more_tiles_than_one_scan_round():
    """More tiles than the scan takes per round (pkg.DECODE_SCAN_ROUND tile sums, from the header),
    so the carry from one round into the next decides every later offset and unit."""
    rng = np.random.default_rng(9)
    n_vals = pkg.DECODE_SCAN_ROUND * T + 77
    n_tiles = (n_vals + T - 1) // T
    assert n_tiles > pkg.DECODE_SCAN_ROUND >= 1024
    lens = rng.integers(0, 4, size=300)
    lens[17] = 0
    tok = [rng.integers(0x20, 0xFFFF, size=l).astype(np.uint16) for l in lens]
    blob = np.concatenate(tok)
    start = np.concatenate([[0], np.cumsum(lens)[:-1]])
    index = rng.permutation(300)[:250].astype(np.int32)
    vals = rng.integers(0, 250, size=n_vals).astype(np.int32)
    cuts = np.sort(rng.integers(0, n_vals + 1, size=4999))
    off = np.concatenate([[0], cuts, [n_vals]]).astype(np.int64)
    # vectorised Python decode: every value's run of blob positions
    ids = index[vals]
    l = lens[ids]
    ends = np.cumsum(l)
    src = np.repeat(start[ids] - (ends - l), l) + np.arange(int(ends[-1]))
    want = blob[src]
    want_off = np.concatenate([[0], ends])[off]
    dec = pkg.Decoder(0)
    try:
        dec.add_tokens(tok)
        dec.set_vector_index(index)
        got, got_off = dec.decode_flat(vals, off, 'vectors')
        assert got_off[-1] == np.sum(lens[index[vals]])
        assert np.array_equal(got_off, want_off)
        assert np.array_equal(got, want)
        # (the last round's tiles: their bases are the carry of the round before plus little)
        tail = int(ends[pkg.DECODE_SCAN_ROUND * T - 1])   # units before the second round's values
        assert 0 < tail < got.size and np.array_equal(got[tail:], want[tail:])
    finally:
        dec.close()


# ---- 4. errors ----------------------------------------------------------------------------------------------

def raw_decode(dec, kind, vals, off, cap):
    """bpe_decode_batch itself, on buffers pre-filled with marks: (rc, units, out_off)."""
    units = np.full(max(cap, 1), 0xABCD, np.uint16)
    out_off = np.full(len(off), -77, np.int64)
    i32p, i64p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)
    rc = pkg.lib().bpe_decode_batch(dec._dec, pkg.Decoder._KINDS[kind], vals.ctypes.data_as(i32p),
                                    off.ctypes.data_as(i64p), len(off) - 1,
                                    units.ctypes.data if cap else None, cap, out_off.ctypes.data_as(i64p))
    return rc, units, out_off


@pytest.mark.gpu
@pytest.mark.parametrize('kind', KINDS)
def test_unknown_values_fail_the_whole_call(edge, kind):
    dec = make_decoder(edge)
    try:
        rng = np.random.default_rng(3)
        n = len(edge['chars'])                            # n_tokens == n_live here
        word = 'token' if kind == 'ids' else 'vector'
        lens = [0, 3, T, 0, T + 20, 5, T - 30, 1]
        good, off = flat([rng.integers(0, 30, size=l).astype(np.int32) for l in lens], lead=2)
        total = int(off[-1] - off[0])
        index = None if kind == 'ids' else edge['index']
        want, want_off = py_decode_flat(good, off, edge['chars'], index)
        need = int(want_off[-1])
        cap = need + 3

        def where(p):                                     # flat position -> (text, position in it)
            k = int(np.searchsorted(off, p + off[0], side='right')) - 1
            return k, int(p + off[0] - off[k])

        for v in (-1, n):
            for p in (0, total - 1, 2 * T + 17):
                bad = good.copy()
                bad[off[0] + p] = v
                rc, units, out_off = raw_decode(dec, kind, bad, off, cap)
                assert rc == pkg.ERR_VOCAB
                assert pkg.last_error() == 'unknown %s index: %d (text %d, position %d)' % ((word, v) + where(p))
                assert (units == 0xABCD).all() and (out_off == -77).all()
                with pytest.raises(pkg.BpeError, match=re.escape('unknown %s index: %d (text' % (word, v))) as ei:
                    dec.decode_flat(bad, off, kind)
                assert ei.value.code == pkg.ERR_VOCAB
        # two bad values: the earlier one is reported
        bad = good.copy()
        bad[off[0] + T + 9] = n + 5
        bad[off[0] + 40] = -3
        rc, units, out_off = raw_decode(dec, kind, bad, off, cap)
        assert rc == pkg.ERR_VOCAB
        assert pkg.last_error() == 'unknown %s index: -3 (text %d, position %d)' % ((word,) + where(40))
        assert (units == 0xABCD).all() and (out_off == -77).all()
        # the decoder stays usable
        got, got_off = dec.decode_flat(good, off, kind)
        assert np.array_equal(got, want) and np.array_equal(got_off, want_off)
        # one unit short: offsets filled, no unit written; with the room it succeeds
        rc, units, out_off = raw_decode(dec, kind, good, off, need - 1)
        assert rc == pkg.ERR_ARG
        assert np.array_equal(out_off, want_off) and (units == 0xABCD).all()
        rc, units, out_off = raw_decode(dec, kind, good, off, need)
        assert rc == pkg.BPE_OK
        assert np.array_equal(out_off, want_off) and np.array_equal(units[:need], want)
        # offsets that are negative (the flat form and add_tokens), and
        with pytest.raises(pkg.BpeError, match='negative text offset') as ei:
            dec.decode_flat(good, np.asarray([-1, 2, 4], np.int64), kind)
        assert ei.value.code == pkg.ERR_ARG
        n_before = dec.num_tokens()
        rc = pkg.lib().bpe_decoder_add_tokens(dec._dec, np.zeros(4, np.uint16).ctypes.data,
                                              np.asarray([-1, 1], np.int64).ctypes.data_as(
                                                  ctypes.POINTER(ctypes.c_int64)), 1)
        assert rc == pkg.ERR_ARG and dec.num_tokens() == n_before
        # offsets that decrease
        with pytest.raises(pkg.BpeError) as ei:
            dec.decode_flat(good, np.asarray([0, 5, 4], np.int64), kind)
        assert ei.value.code == pkg.ERR_ARG
    finally:
        dec.close()


@pytest.mark.gpu
def test_index_state_and_merge_checks(edge):
    dec = pkg.Decoder(0)
    try:
        dec.add_tokens(['a', 'b', 'c'])
        with pytest.raises(pkg.BpeError) as ei:           # vectors without an index
            dec.decode([[0, 1]], 'vectors')
        assert ei.value.code == pkg.ERR_STATE
        assert dec.decode([[0, 1]], 'ids') == ['ab']
        dec.set_vector_index([2, 0])
        assert dec.decode([[0, 1, 1]], 'vectors') == ['caa']
        with pytest.raises(pkg.BpeError) as ei:           # an index naming an unknown token
            dec.set_vector_index([0, 3])
        assert ei.value.code == pkg.ERR_VOCAB
        assert dec.decode([[0, 1, 1]], 'vectors') == ['caa']
        dec.add_merges([(0, 1, 3)])                       # drops the index
        with pytest.raises(pkg.BpeError) as ei:
            dec.decode([[0]], 'vectors')
        assert ei.value.code == pkg.ERR_STATE
        dec.set_vector_index([3, 2])
        assert dec.decode([[0, 1, 0]], 'vectors') == ['abcab']
        dec.set_vector_index(None)                        # n == 0 with NULL drops it
        with pytest.raises(pkg.BpeError) as ei:
            dec.decode([[0]], 'vectors')
        assert ei.value.code == pkg.ERR_STATE
        dec.set_vector_index([3])
        dec.add_tokens(['d'])                             # drops it as well; ids interleave
        with pytest.raises(pkg.BpeError) as ei:
            dec.decode([[0]], 'vectors')
        assert ei.value.code == pkg.ERR_STATE
        assert dec.num_tokens() == (5, 6)
        for abc, code in [([(0, 1, 6)], pkg.ERR_ARG),               # c != count
                          ([(0, 1, 4)], pkg.ERR_ARG),
                          ([(0, 5, 5)], pkg.ERR_VOCAB),             # a or b >= count
                          ([(5, 0, 5)], pkg.ERR_VOCAB),
                          ([(-1, 0, 5)], pkg.ERR_VOCAB),
                          ([(0, 1, 5), (5, 7, 6)], pkg.ERR_VOCAB),  # the first triple is fine
                          ([(0, 1, 5), (5, 5, 7)], pkg.ERR_ARG)]:
            with pytest.raises(pkg.BpeError) as ei:
                dec.add_merges(abc)
            assert ei.value.code == code, abc
            assert dec.num_tokens() == (5, 6)             # a failed call adds nothing
        dec.add_merges([(4, 3, 5), (5, 5, 6)])            # b names a token of the same call
        assert dec.decode([[6, 4]], 'ids') == ['dabdabd']
        dec.clear()
        assert dec.num_tokens() == (0, 0)
        dec.add_tokens(['x', np.asarray([0xD83D, 0xDE00], np.uint16), '\udc00'])
        assert dec.decode([[2, 1, 0]], 'ids') == ['\udc00\U0001F600x']
    finally:
        dec.close()


# ---- 5. with the engine and the encoder ----------------------------------------------------------------

@pytest.mark.gpu
def test_round_trip_with_engine_and_encoder():
    data = pkg.synth_latin1(64 << 10, A=95)
    e = pkg.Engine(0)
    dec = pkg.Decoder(0)
    try:
        cmap, nt, _hist = e.add_latin1(data, sample_bytes=4096)
        assert nt == 95
        merges = e.merge_until(0, 2, 300)
        assert len(merges) == 300
        abc = [(a, b, nt + k) for k, (a, b, _w) in enumerate(merges)]
        seen = np.nonzero(cmap >= 0)[0]
        byte_of = np.zeros(nt, np.int64)
        byte_of[cmap[seen]] = seen
        dec.add_tokens([chr(int(b)) for b in byte_of])
        dec.add_merges(abc)
        ids, off = e.read_corpus()
        assert len(off) - 1 == 16 and len(ids) < len(data)
        units, out_off = dec.decode_flat(ids, off, 'ids')
        for k in range(16):
            assert units[out_off[k]:out_off[k + 1]].tobytes() == \
                data[4096 * k:4096 * (k + 1)].astype(np.uint16).tobytes(), k
        rng = np.random.default_rng(1)
        texts = [rng.integers(0, 95, size=rng.integers(0, 400)).astype(np.uint8) for _ in range(200)]
        enc = pkg.Encoder(0, abc)
        try:
            coded = enc.encode([cmap[t] for t in texts])
        finally:
            enc.close()
        assert sum(len(c) for c in coded) < sum(len(t) for t in texts)
        assert dec.decode(coded, 'ids') == [bytes(t).decode('latin1') for t in texts]
    finally:
        dec.close()
        e.close()


# ---- 6. the device form --------------------------------------------------------------------------------------

def device_form_check(kind):
    """The batch of test 2 through decode_tensors: equal to the host form.  Returns False when
    torch sees no device."""
    import torch
    if not torch.cuda.is_available():
        return False
    edge = make_edge()
    dec = make_decoder(edge)
    try:
        dev = torch.device('cuda', 0)
        vals, off = batch_of(edge, kind, lead=5)
        want, want_off = dec.decode_flat(vals, off, kind)
        index = None if kind == 'ids' else edge['index']
        assert np.array_equal(want, py_decode_flat(vals, off, edge['chars'], index)[0])
        # the value buffer at every 16-B misalignment (a slice of a larger tensor)
        for shift in range(4):
            buf = torch.from_numpy(np.concatenate([np.full(shift, -9, np.int32), vals])).to(dev)
            units, out_off = dec.decode_tensors(buf[shift:], torch.from_numpy(off).to(dev), kind)
            assert units.dtype == torch.int16 and out_off.dtype == torch.int64 and units.is_cuda
            assert np.array_equal(out_off.cpu().numpy(), want_off), shift
            assert np.array_equal(units.cpu().numpy().view(np.uint16), want), shift
        # the output buffer at every 16-B misalignment, through the entry point itself: runs
        # shifted by it, and nothing written before or after the units
        d_off = torch.from_numpy(off).to(dev)
        d_vals = torch.from_numpy(vals).to(dev)
        for shift in (1, 3, 7):
            room = torch.full((shift + want.size + 9,), 0x5A5A, dtype=torch.int16, device=dev)
            out_off = torch.full((len(off),), -77, dtype=torch.int64, device=dev)
            need = ctypes.c_int64()
            torch.cuda.synchronize(dev)
            rc = pkg.lib().bpe_decode_batch_device(dec._dec, pkg.Decoder._KINDS[kind], d_vals.data_ptr(),
                                                   d_off.data_ptr(), len(off) - 1,
                                                   room[shift:].data_ptr(), want.size,
                                                   out_off.data_ptr(), ctypes.byref(need))
            assert rc == pkg.BPE_OK and need.value == want.size, (shift, pkg.last_error())
            h = room.cpu().numpy().view(np.uint16)
            assert (h[:shift] == 0x5A5A).all() and (h[shift + want.size:] == 0x5A5A).all(), shift
            assert np.array_equal(h[shift:shift + want.size], want), shift
            assert np.array_equal(out_off.cpu().numpy(), want_off), shift
        # an unknown value on the device
        bad = torch.from_numpy(vals).to(dev)
        bad[int(off[0]) + T + 3] = -2
        with pytest.raises(pkg.BpeError, match=r'unknown \w+ index: -2 \(text') as ei:
            dec.decode_tensors(bad, torch.from_numpy(off).to(dev), kind)
        assert ei.value.code == pkg.ERR_VOCAB
        empty = dec.decode_tensors(torch.zeros(0, dtype=torch.int32, device=dev),
                                   torch.zeros(1, dtype=torch.int64, device=dev), kind)
        assert empty[0].numel() == 0 and empty[1].tolist() == [0]
    finally:
        dec.close()
    return True


@pytest.mark.gpu
def test_device_form_equals_host_form():
    """In a process of its own that imports torch before libbpe loads: PyTorch sees a device only
    when its HIP runtime is the process's first (pytest's collection loads libbpe first)."""
    pytest.importorskip('torch')
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join(
        [here, os.path.join(os.path.dirname(here), 'oracle'), os.environ.get('PYTHONPATH', '')]))
    out = subprocess.run([sys.executable, os.path.abspath(__file__), 'device-form'], env=env,
                         capture_output=True, text=True, timeout=300)
    if out.returncode == 0 and out.stdout.strip().endswith('no device'):
        pytest.skip('torch sees no device')
    assert out.returncode == 0 and out.stdout.strip().endswith('device form ok'), \
        out.stdout[-2000:] + out.stderr[-3000:]


# ---- 7. CPU ------------------------------------------------------------------------------------------------------

def test_decoder_needs_a_device_and_the_abi_names_it():
    L = pkg.lib()
    assert L.bpe_version() == 201
    for name in ('bpe_decoder_create', 'bpe_decode_batch', 'bpe_decode_batch_device'):
        assert name in pkg.C_API and hasattr(L, name)
    assert T == 1024 and ctypes.sizeof(pkg.DecoderStats) == 40
    if pkg.device_count() == 0:
        with pytest.raises(pkg.BpeError, match='no HIP device') as ei:
            pkg.Decoder(0)
        assert ei.value.code == pkg.ERR_HIP
    else:
        pkg.Decoder(0).close()


if __name__ == '__main__' and sys.argv[1:] == ['device-form']:
    import torch  # noqa: F401  (before libbpe loads)
    print('device form ok' if all([device_form_check(k) for k in KINDS]) else 'no device')
