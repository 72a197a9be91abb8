"""fast_tier_kernel's record read (rec_xpose.h): each wave loads its 64
records of a group as three coalesced 1-KB instructions and an in-wave
transpose hands lane q its record.  The edges of that mapping are not those
of the decision (tests/test_gpu_boundaries.py): in 16-byte chunks, 3n meets
an instruction edge at n = 21 / 22 (64), 42 / 43 (128) and 64 (192), a wave
edge at every 64 records, a record-group edge at every 256 (277 / 278: 64
chunks into the second group), and the key's first chunk sits at any of the
eight 16-byte places of a 128-byte line.

Keys are tests/planted.py's: every invalid one has its valid twin in the same
batch.  Every key, no mask: verdict, fail op and failing prefix end equal the
CPU oracle's JITC search, through lc_check_device with the launched kernel
(LC_RESIDENT=0) and with the default path, which agree field for field.
tests/test_record_transpose_plants.py pins the oracle's answers to the
plants' construction without a GPU."""
import functools

import numpy as np
import pytest

import oracle
import planted
from helpers import pack_keys
from test_resident import FIELDS, _dev, _launched, _run

pytestmark = pytest.mark.gpu

# 3n at an instruction, wave or record-group edge of the chunk mapping
LENGTHS = (1, 2, 3, 21, 22, 42, 43, 63, 64, 65, 128, 192, 255, 256, 257, 277, 278, 1023, 1024)
# the deciding record of a 1,024-record ladder: every lane of one wave, and
# either side of every record-group edge
RECORDS = tuple(range(64)) + (255, 256, 511, 512, 767, 768, 1023)
GROUPS = ("lengths", "records", "aligned")


def _pairs(n, re, p):
    """Invalid plants whose deciding record is at position / record p of the
    n-record ladder, each followed by its valid twin."""
    m = planted.n_positions(n, re)
    out = []
    if p < m:
        out += [planted.cas_exp(n, re, p), planted.cas_exp(n, re, p, good=True)]
    if p < n:
        out += [planted.read_val(n, re, p), planted.read_val(n, re, p, good=True)]
    if 1 <= p < m:  # the write at position p claims version p: Own[p - 1] held twice
        out += [planted.dup(n, re, p - 1), planted.base(n, re)]
    if p + 1 < m:  # versions of positions p, p + 1 exchanged: fails at the holder of p
        out += [planted.swap(n, re, p), planted.base(n, re)]
    return out


def _unique(plants):
    seen, out = set(), []
    for pl in plants:
        if pl.tag not in seen:
            seen.add(pl.tag)
            out.append(pl)
    return out


def _aligned():
    """Tested keys starting at record offsets = 0 .. 7 (mod 8), that is at
    every 16-byte place of a 128-byte line (48 r mod 128 = 16 (3 r mod 8)),
    each behind a filler ladder of 1 .. 7 records where one is needed."""
    tested = []
    for i, n in enumerate((1024, 1000, 277, 65, 1023, 256, 43, 999)):
        p = (0, n - 1, n // 2, 63, 64, 21, n - 2, 500)[i] % n
        tested.append(_pairs(n, 0, p)[:2] + _pairs(n, 0, p)[-2:])
    out, off = [], 0
    for a in range(8):
        for pl in tested[a]:
            fill = (a - off) % 8
            if fill:
                out.append(planted.base(fill))
                off += fill
            assert off % 8 == a
            out.append(pl)
            off += len(pl.recs)
    return out


@functools.lru_cache(maxsize=None)
def batch(name):
    """(plants, ops, key_off, oracle results) of one group, computed once and
    left unchanged."""
    if name == "lengths":
        pls = []
        for n in LENGTHS:
            for re in (0, 3):
                pls.append(planted.base(n, re))
                for p in sorted({0, n // 2, n - 2, n - 1} & set(range(n))):
                    pls += _pairs(n, re, p)
        pls = planted.interleave(_unique(pls))
    elif name == "records":
        pls = []
        for p in RECORDS:
            pls += _pairs(1024, 0, p)
        pls = _unique(pls)
    else:
        pls = _aligned()
    ops, off = pack_keys([pl.recs for pl in pls])
    _, j = oracle.check(ops, off, algo=oracle.JITC, n_threads=16)
    assert (j["verdict"] == [pl.verdict for pl in pls]).all()
    assert (j["fail_op"] == [pl.fail_op for pl in pls]).all()
    return pls, ops, off, j


def _same(pls, got, want, fields, what):
    for f in fields:
        bad = np.nonzero(got[f] != want[f])[0]
        assert len(bad) == 0, (what, f, len(bad), [(pls[k].tag, int(got[f][k]), int(want[f][k]))
                                                   for k in bad[:8]])


def _both(ctx, monkeypatch, pls, d_ops, d_off, j):
    """The launched kernel against the oracle, then the default path against
    the launched kernel in every result field."""
    monkeypatch.setenv("LC_FUSED", "0")  # (the version-order pass, whatever the call before chose)
    want = _launched(ctx, d_ops, d_off, len(pls), monkeypatch)
    _same(pls, want, j, ("verdict", "fail_op", "fail_prefix_end"), "launched")
    _same(pls, _run(ctx, d_ops, d_off, len(pls)), want, FIELDS, "default")


def test_every_invalid_key_has_its_valid_twin():
    for name in GROUPS:
        pls = batch(name)[0]
        tags = {pl.tag for pl in pls if pl.verdict == 1}
        for pl in pls:
            if pl.verdict == 0:
                n, re = int(pl.tag.split(" n=")[1].split()[0]), int(pl.tag.split(" re=")[1].split()[0])
                twin = pl.tag.replace("good=0", "good=1") if "good=0" in pl.tag else planted.base(n, re).tag
                assert twin in tags, pl.tag


@pytest.mark.parametrize("name", GROUPS)
def test_equals_the_oracle_launched_and_default(ctx, monkeypatch, name):
    pls, ops, off, j = batch(name)
    _both(ctx, monkeypatch, pls, _dev(ops), _dev(off), j)


def test_sub_range_of_the_aligned_batch(ctx, monkeypatch):
    """The same device buffers from key a on: the records' and the offsets'
    pointers advanced, so key_off[0] != 0, and the first key starts at another
    place of its line than the buffer does."""
    pls, ops, off, j = batch("aligned")
    d_ops, d_off = _dev(ops), _dev(off)
    firsts = [k for k in range(1, len(pls)) if off[k] % 8 in (3, 6)][:2]
    assert len(firsts) == 2
    for a in firsts:
        _both(ctx, monkeypatch, pls[a:], d_ops[int(off[a]):], d_off[a:], j[a:])
