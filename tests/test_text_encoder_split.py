"""The text form on the split route (bpe_encode_text_batch and its device form with
BPE_LONG_SPLIT): a text of more than ENCODE_LDS_TOKENS chars is planned on the front end's ids and
stays on the device through the vector index and the pack.  Values are checked against the id
form's yardstick on the mapped chars (oracle.encode, then the index), the split stats against the
Python plan of tests/test_encoder_split.py, and the errors against the messages include/bpe.h
names, with positions relative to the text.
"""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from bpe_amd import pkg
from test_encoder_split import CAP, fixture_a, plan_stats, planted

KINDS = ['ids', 'vectors']
SENTINEL = 0x7EADBEEF
BMP = 'abcdefghi'                                             # ids 0..8
PAIR = '\U0001F600'                                           # id 9: two units, one char
JUNK = 0x1234                                                 # a unit the table does not know


def vocab():
    merges = fixture_a()
    table = {c: i for i, c in enumerate(BMP)}
    table[PAIR] = 9
    index = np.random.default_rng(13).permutation(10 + len(merges)).astype(np.int32)
    return dict(merges=merges, table=table, index=index)


def units_of_ids(ids):
    """The UTF-16 units of a text given as ids 0..9 (id 9: the pair)."""
    ids = np.asarray(ids)
    pair = np.frombuffer(PAIR.encode('utf-16-le'), dtype='<u2')
    out = np.empty(len(ids) + int((ids == 9).sum()), np.uint16)
    at = np.arange(len(ids)) + np.concatenate([[0], np.cumsum(ids == 9)[:-1]]) if len(ids) else np.zeros(0, int)
    out[at] = np.where(ids == 9, pair[0], ord('a') + np.minimum(ids, 8))
    out[at[ids == 9] + 1] = pair[1]
    return out


def flat(rows, lead=0):
    off = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=off[1:])
    units = np.concatenate([np.full(lead, JUNK, np.uint16)] + [np.asarray(r, np.uint16) for r in rows])
    return units.astype(np.uint16), off + lead


@functools.lru_cache(maxsize=None)
def batch():
    """A short text, a BMP text of cap + 1 chars that splits (its 9 past the first segment), a
    pair text of cap + 2 units (cap / 2 + 1 chars: not long once counted in chars), an empty text,
    a second long text, a short text; with the id form's outputs."""
    rng = np.random.default_rng(14)
    long0 = planted(rng, CAP + 1, [5000, 12000])
    long0[9000] = 9
    long1 = planted(rng, 2 * CAP + 3, range(1000, 2 * CAP, 3000))
    ids = [planted(rng, 50, [7]), long0, np.full(CAP // 2 + 1, 9, np.int32), np.zeros(0, np.int32),
           long1, planted(rng, 700, [])]
    rows = [units_of_ids(t) for t in ids]
    assert len(rows[1]) == CAP + 2 and len(rows[2]) == CAP + 2
    return ids, rows, oracle.encode(ids, fixture_a())


def make_encoder(v, mode='split'):
    enc = pkg.Encoder(0, v['merges'], long_texts=mode)
    enc.set_chars(v['table'])
    enc.set_vector_index(v['index'])
    return enc


def want_values(v, want_ids, kind):
    vals = np.concatenate(want_ids).astype(np.int32)
    off = np.concatenate([[0], np.cumsum([len(w) for w in want_ids])]).astype(np.int64)
    return (v['index'][vals] if kind == 'vectors' else vals), off


def raw_text(enc, kind, units, off):
    """bpe_encode_text_batch itself, on outputs pre-filled with marks: (rc, vals, out_off)."""
    cap = int(off[-1] - off[0])
    vals = np.full(max(cap, 1), SENTINEL, np.int32)
    out_off = np.full(len(off), -77, np.int64)
    rc = pkg.lib().bpe_encode_text_batch(enc._enc, pkg.Encoder._KINDS[kind], units.ctypes.data,
                                         off.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), len(off) - 1,
                                         vals.ctypes.data, cap,
                                         out_off.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)))
    return rc, vals, out_off


@pytest.mark.gpu
@pytest.mark.parametrize('kind', KINDS)
def test_host_form_splits_and_stays_on_the_device(kind):
    v = vocab()
    ids, rows, want_ids = batch()
    want, want_off = want_values(v, want_ids, kind)
    exp, _plans = plan_stats(ids, v['merges'])
    assert exp['texts_split'] == 2 and exp['texts_fallback'] == 0
    enc = make_encoder(v)
    try:
        for lead in (0, 5):
            units, off = flat(rows, lead)
            enc.reset_stats()
            enc.reset_split_stats()
            got, got_off = enc.encode_text_flat(units, off, kind)
            assert np.array_equal(got_off, want_off) and np.array_equal(got, want), lead
            st, ss = enc.stats(), enc.split_stats()
            assert st['texts_replay'] == 0 and st['texts_rank'] == len(rows)
            assert {k: ss[k] for k in exp} == exp and ss['calls'] == 1
        # the default route on the same batch: the whole call through the replay, equal values
        enc.set_long_texts('replay')
        enc.reset_stats()
        enc.reset_split_stats()
        got, got_off = enc.encode_text_flat(*flat(rows), kind)
        assert np.array_equal(got_off, want_off) and np.array_equal(got, want)
        assert enc.stats()['texts_replay'] == 2 and enc.split_stats()['windows'] == 0
    finally:
        enc.close()


@pytest.mark.gpu
def test_a_text_without_a_boundary_sends_the_call_through_the_replay():
    v = vocab()
    rng = np.random.default_rng(15)
    ids = [planted(rng, CAP + 1, [77]), planted(rng, CAP + 9, []), planted(rng, 30, [])]
    want_ids = oracle.encode(ids, v['merges'])
    enc = make_encoder(v)
    try:
        for kind in KINDS:
            want, want_off = want_values(v, want_ids, kind)
            enc.reset_stats()
            enc.reset_split_stats()
            got, got_off = enc.encode_text_flat(*flat([units_of_ids(t) for t in ids]), kind)
            assert np.array_equal(got_off, want_off) and np.array_equal(got, want)
            st, ss = enc.stats(), enc.split_stats()
            assert st['texts_replay'] == 1 and st['texts_rank'] == 2
            assert (ss['calls'], ss['texts_split'], ss['texts_fallback'], ss['segments']) == (1, 1, 1, 2)
    finally:
        enc.close()


@pytest.mark.gpu
@pytest.mark.parametrize('kind', KINDS)
def test_unknown_char_past_the_first_segment(kind):
    v = vocab()
    _ids, rows, want_ids = batch()
    enc = make_encoder(v)
    try:
        for at in (9000, CAP):                                # (the second segment, the last one)
            bad = [r.copy() for r in rows]
            bad[1][at] = ord('z')
            units, off = flat(bad, 3)
            rc, vals, out_off = raw_text(enc, kind, units, off)
            assert rc == pkg.ERR_VOCAB
            assert pkg.last_error() == 'unknown token, char: U+007A (text 1, unit %d)' % at
            assert (vals == SENTINEL).all() and (out_off == -77).all()
        want, want_off = want_values(v, want_ids, kind)
        got, got_off = enc.encode_text_flat(*flat(rows), kind)   # the encoder stays usable
        assert np.array_equal(got_off, want_off) and np.array_equal(got, want)
    finally:
        enc.close()


@pytest.mark.gpu
def test_hole_past_the_first_segment_and_the_error_order():
    """A hole at id 9: the long text's 9 lies in its second segment, and its position is counted
    from the text's start; the pair text after it (all 9s) fails later, so text 1's error is the
    call's.  An unknown char in an earlier text comes first; one in a later text does not."""
    v = vocab()
    _ids, rows, want_ids = batch()
    index = v['index'].copy()
    index[9] = -1
    pos = want_ids[1].tolist().index(9)
    first_seg = len(oracle.encode([_ids[1][:5001]], v['merges'])[0])
    assert pos >= first_seg                                   # (past the first segment's output)
    enc = make_encoder(v)
    try:
        enc.set_vector_index(index)
        units, off = flat(rows)
        rc, vals, out_off = raw_text(enc, 'vectors', units, off)
        assert rc == pkg.ERR_VOCAB and pkg.last_error() == 'unknown token index: 9 (text 1, position %d)' % pos
        assert (vals == SENTINEL).all() and (out_off == -77).all()
        for k, msg in ((0, 'unknown token, char: U+007A (text 0, unit 3)'),
                       (5, 'unknown token index: 9 (text 1, position %d)' % pos)):
            bad = [r.copy() for r in rows]
            bad[k][3] = ord('z')
            rc, vals, out_off = raw_text(enc, 'vectors', *flat(bad))
            assert rc == pkg.ERR_VOCAB and pkg.last_error() == msg
            assert (vals == SENTINEL).all() and (out_off == -77).all()
        got, got_off = enc.encode_text_flat(units, off, 'ids')   # ids need no index
        want, want_off = want_values(v, want_ids, 'ids')
        assert np.array_equal(got_off, want_off) and np.array_equal(got, want)
    finally:
        enc.close()


# ---- the device form, in a process that imports torch first ----------------------------------------------

def device_form_check():
    import torch
    if not torch.cuda.is_available():
        return False
    dev = torch.device('cuda', 0)
    v = vocab()
    ids, rows, want_ids = batch()
    exp, _plans = plan_stats(ids, v['merges'])
    enc = make_encoder(v)
    try:
        for kind in KINDS:
            want, want_off = want_values(v, want_ids, kind)
            for lead in (0, 3):
                units, off = flat(rows, lead)
                d_units = torch.from_numpy(units.view(np.int16)).to(dev)
                enc.reset_stats()
                enc.reset_split_stats()
                vals, out_off = enc.encode_text_tensors(d_units, torch.from_numpy(off).to(dev), kind)
                assert vals.is_cuda and out_off.is_cuda
                assert np.array_equal(out_off.cpu().numpy(), want_off), (kind, lead)
                assert np.array_equal(vals.cpu().numpy(), want), (kind, lead)
                ss = enc.split_stats()
                assert enc.stats()['texts_replay'] == 0 and {k: ss[k] for k in exp} == exp
        # errors on the device: nothing written, positions relative to the text
        bad = [r.copy() for r in rows]
        bad[1][9000] = ord('z')
        units, off = flat(bad)
        d_vals = torch.full((len(units),), SENTINEL, dtype=torch.int32, device=dev)
        d_ooff = torch.full((len(off),), -77, dtype=torch.int64, device=dev)
        d_units, d_off = torch.from_numpy(units.view(np.int16)).to(dev), torch.from_numpy(off).to(dev)
        need = ctypes.c_int64()
        torch.cuda.synchronize(dev)
        rc = pkg.lib().bpe_encode_text_batch_device(enc._enc, pkg.ENCODE_VECTORS, d_units.data_ptr(), d_off.data_ptr(),
                                                    len(off) - 1, d_vals.data_ptr(), len(units), d_ooff.data_ptr(),
                                                    ctypes.byref(need))
        assert rc == pkg.ERR_VOCAB and pkg.last_error() == 'unknown token, char: U+007A (text 1, unit 9000)'
        assert bool((d_vals == SENTINEL).all()) and bool((d_ooff == -77).all())
        index = v['index'].copy()
        index[9] = -1
        enc.set_vector_index(index)
        units, off = flat(rows)
        d_units = torch.from_numpy(units.view(np.int16)).to(dev)
        pos = want_ids[1].tolist().index(9)
        with pytest.raises(pkg.BpeError, match=r'unknown token index: 9 \(text 1, position %d\)' % pos):
            enc.encode_text_tensors(d_units, torch.from_numpy(off).to(dev), 'vectors')
        enc.set_vector_index(v['index'])
        vals, out_off = enc.encode_text_tensors(d_units, torch.from_numpy(off).to(dev), 'vectors')
        assert np.array_equal(vals.cpu().numpy(), want_values(v, want_ids, 'vectors')[0])
    finally:
        enc.close()
    return True


@pytest.mark.gpu
def test_device_form():
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


# ---- CPU ------------------------------------------------------------------------------------------------

def test_units_of_ids_is_one_char_per_id():
    ids = np.asarray([0, 9, 8, 9, 9, 3], np.int32)
    assert pkg.units_to_str(units_of_ids(ids)) == 'a' + PAIR + 'i' + PAIR + PAIR + 'd'
    assert len(units_of_ids(np.zeros(0, np.int32))) == 0


if __name__ == '__main__' and sys.argv[1:] == ['device-form']:
    import torch  # noqa: F401  (before libbpe loads)
    print('device form ok' if device_form_check() else 'no device')
