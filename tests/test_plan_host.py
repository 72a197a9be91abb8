"""csrc/plan_host.h and plan_host.cpp, the register path's host arithmetic:
tests/plan_main.cpp built with g++ and the address and undefined-behaviour
sanitizers, run as a child process (as tests/test_workspace.py runs its
program).  The program plans chunks and device splits, packs records to 24 and
16 bytes and cuts counted classes; its lines carry the raw plans, judged
here."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
WIDTHS = (16, 24, 48)
CHUNK_CASES = ("one_key", "all_empty", "tail_minus", "tail", "tail_plus", "max_chunks", "empty_ends")
DEVICE_CASES = ("nd1", "nd2", "nd8", "more_devices_than_keys", "irregular_at_0", "irregular_unprobed")


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed"
    exe = str(tmp_path_factory.mktemp("plan") / "plan_main")
    # the sanitizers' runtimes linked in statically: the program needs no place in anybody's preload list
    subprocess.check_call([cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           os.path.join(HERE, "plan_main.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return [ln.split() for ln in r.stdout.splitlines()]


@pytest.fixture(scope="module")
def consts(lines):
    (f,) = [f for f in lines if f[0] == "const"]
    return dict(zip(("chunk_bytes", "chunk_tail", "max_chunks", "key_stride", "sample_stride"), map(int, f[1:])))


def _ints(f, a, b=None):
    i = f.index(a) + 1
    return [int(x) for x in f[i:f.index(b) if b else len(f)]]


@pytest.fixture(scope="module")
def chunks(lines):
    out = {}
    for f in lines:
        if f[0] == "chunks":
            out[f[1], int(f[2])] = dict(nk=int(f[3]), n=int(f[4]), k=_ints(f, "k", "r"), r=_ints(f, "r", "want"),
                                        want=_ints(f, "want"))
    return out


def test_every_chunk_case_ran(chunks):
    assert sorted(chunks) == sorted((c, w) for c in CHUNK_CASES for w in WIDTHS)


@pytest.mark.parametrize("rec", WIDTHS)
@pytest.mark.parametrize("case", CHUNK_CASES)
def test_plan_chunks(chunks, consts, case, rec):
    p = chunks[case, rec]
    k, n = p["k"], p["n"]
    assert len(k) == len(p["r"]) == n + 1
    assert k[0] == 0 and k[n] == p["nk"]
    assert all(a < b for a, b in zip(k, k[1:])), k
    assert p["r"] == p["want"]  # r[i] == off[k[i]] - off[0]
    assert 1 <= n <= consts["max_chunks"]


@pytest.mark.parametrize("rec", WIDTHS)
def test_plan_chunks_sizes(chunks, consts, rec):
    """What the cases are there for: input up to kChunkTail is one chunk; the
    large input runs into kMaxChunks, its chunks (cut at key boundaries, a key
    is 4 Ki records) at most kChunkBytes and a key, the last one at most
    kChunkTail; empty keys at the ends join the first and last chunk."""
    for case in ("one_key", "all_empty", "tail_minus", "tail"):
        assert chunks[case, rec]["n"] == 1
    assert chunks["tail_plus", rec]["n"] <= 2
    # 1200 MiB is more than kMaxChunks - 1 chunks hold (2 + 4 + 8 + 16 + 43 x 24 MiB): the first chunk
    # takes what is over; every other chunk starts at the first key boundary at or past its byte goal
    big = chunks["max_chunks", rec]
    assert consts["max_chunks"] - 1 <= big["n"] <= consts["max_chunks"]
    sizes = [rec * (b - a) for a, b in zip(big["r"], big["r"][1:])]
    key = rec << 12
    assert sizes[0] > consts["chunk_bytes"] + key
    assert max(sizes[1:]) <= consts["chunk_bytes"] + key
    assert sizes[-1] <= consts["chunk_tail"]
    ends = chunks["empty_ends", rec]
    assert ends["n"] > 1 and ends["k"][1] > 3 and ends["k"][-2] < ends["nk"] - 4


@pytest.fixture(scope="module")
def devices(lines):
    out = {}
    for f in lines:
        if f[0] == "devices":
            out[f[1], int(f[2])] = dict(nd=int(f[3]), n_keys=int(f[4]), bounds=_ints(f, "bounds", "len"),
                                        lens=_ints(f, "len"))
    return out


def _by_record_count(lens, nd):
    """plan_devices' cut when every key costs its record count + 64."""
    pre = [0.0]
    for n in lens:
        pre.append(pre[-1] + n + 64.0)
    bounds, k = [0], 0
    for p in range(1, nd):
        goal = pre[-1] * p / nd
        while k < len(lens) and pre[k] < goal:
            k += 1
        bounds.append(k)
    return bounds + [len(lens)]


@pytest.mark.parametrize("rec", (24, 48))
@pytest.mark.parametrize("case", DEVICE_CASES)
def test_plan_devices(devices, consts, case, rec):
    p = devices[case, rec]
    b = p["bounds"]
    assert len(b) == p["nd"] + 1 and len(p["lens"]) == p["n_keys"]
    assert b[0] == 0 and b[-1] == p["n_keys"]
    assert all(x <= y for x, y in zip(b, b[1:])), b
    if case == "irregular_at_0":
        # the probe finds key 0, which is priced as a crashed key: the first share ends earlier
        assert b != _by_record_count(p["lens"], p["nd"]) and b[1] < _by_record_count(p["lens"], p["nd"])[1]
    else:
        # nothing irregular, or the one irregular key not at a multiple of kKeyStride: by record count
        assert (consts["key_stride"] + 5) % consts["key_stride"]
        assert b == _by_record_count(p["lens"], p["nd"])


def test_pack_round_trip(lines):
    got = {(f[1], f[2]): tuple(map(int, f[3:6])) for f in lines if f[0] == "pack"}
    erange = -34
    assert got == {
        # (case, width): (rc, records, records with widen_op(pack(x)) == x)
        ("ids_at_max", "32"): (0, 7, 7), ("ids_at_max", "16"): (0, 7, 7), ("ids_at_max", "inf32"): (0, 1, 1),
        ("ids_past_max", "32"): (0, 7, 7), ("ids_past_max", "16"): (erange, 7, 0),
        ("ids_past_max", "inf32"): (0, 1, 1),
        ("no_keys", "32"): (0, 0, 0), ("no_keys", "16"): (0, 0, 0)}


def test_counted_classes_agree(lines):
    got = {}
    for f in lines:
        if f[0] == "counted":
            got[f[1]] = dict(rc=int(f[3]), n_classes=int(f[5]), fits=int(f[7]), take=int(f[9]),
                             plan=f[f.index("plan") + 1:f.index("host")], host=f[f.index("host") + 1:])
    a, b = got["classes16"], got["classes17"]
    assert a["rc"] == b["rc"] == 0
    assert a["n_classes"] == 16 and a["fits"] == a["take"] == 1
    assert a["plan"] == a["host"] and len(a["plan"]) == 16  # class order (value) and member counts
    assert sorted(set(m.split(":")[1] for m in a["plan"])) == ["1", "2", "3"]
    assert b["n_classes"] == 17 and b["take"] == 0 and b["fits"] == b["take"]
