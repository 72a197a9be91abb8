"""csrc/watch_host.cpp: tests/watch_main.cpp built with g++ and the address and
undefined-behaviour sanitizers, run as a child process (as
tests/test_wr_host_sanitize.py runs its program).  The program checks the
KATs' arrays and inputs this test generates, then inputs of its own, every
input and output array sized exactly; its lines carry each call's counts, which
must be those the library gives through the binding."""
import json
import os
import random
import shutil
import struct
import subprocess

import numpy as np
import pytest

from jepsen.etcd_amd import abi, watch as W

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "jepsen", "etcd_amd", "csrc")
KATS = json.load(open(os.path.join(HERE, "golden", "watch_kat.json")))["cases"]
FIELDS = (("valid", "valid"), ("canonical", "canonical"), ("size", "canonical_size"), ("threads", "n_threads"),
          ("classes", "n_classes"), ("deltas", "n_deltas"), ("edits", "n_edits"), ("noscript", "n_no_script"),
          ("collisions", "n_collisions"), ("reveq", "revisions_equal"))


def inputs():
    """The KATs' arrays, then generated ones: (threads, values, n_nonmonotonic)."""
    out = []
    for kat in KATS:
        enc = W.encode(kat["history"], kat["concurrency"])
        out.append((enc.threads, enc.values, len(enc.nonmonotonic)))
    rng = random.Random(0xA5A)
    for i in range(40):
        n, edits = rng.randint(0, 300), {t: rng.randint(1, 5) for t in range(1, rng.randint(1, 7), 2)}
        threads, values = W.synth_arrays(rng.randint(2, 8), n, edits, seed=i)
        if i % 4 == 0:
            values = values % 2  # few symbols: long common runs, prefixes and suffixes that would overlap
        out.append((threads, values, int(i % 7 == 0)))
    return out


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed"
    tmp = tmp_path_factory.mktemp("watch")
    exe, cases = str(tmp / "watch_main"), str(tmp / "cases.bin")
    ins = inputs()
    with open(cases, "wb") as f:
        f.write(struct.pack("<q", len(ins)))
        for threads, values, nn in ins:
            f.write(struct.pack("<qqq", len(threads), len(values), nn))
            f.write(np.ascontiguousarray(threads, dtype=abi.WT_THREAD_DTYPE).tobytes())
            f.write(np.ascontiguousarray(values, dtype=np.int64).tobytes())
    # the sanitizers' runtimes linked in statically: the program needs no place in anybody's preload list
    subprocess.check_call([cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", CSRC,
                           os.path.join(HERE, "watch_main.cpp"), os.path.join(CSRC, "watch_host.cpp"), "-o", exe])
    env = {k: v for k, v in os.environ.items() if not k.startswith("LC_WT_")}
    r = subprocess.run([exe, cases], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    out = []
    for ln in r.stdout.splitlines():
        f = ln.split()
        out.append((f[0], int(f[1]), dict(zip(f[2::2], f[3::2]))))
    return out


def test_cases_under_the_sanitizers_give_the_library_s_counts(lines):
    cases = [rec for name, _, rec in lines if name == "case"]
    ins = inputs()
    assert len(cases) == len(ins)
    seen_edits = 0
    for i, ((threads, values, nn), rec) in enumerate(zip(ins, cases)):
        out, s = abi.watch_check_host(threads, values, nn)
        assert int(rec["rc"]) == 0, i
        assert [int(rec[a]) for a, _ in FIELDS] == [s[b] for _, b in FIELDS], (i, rec, s)
        assert int(rec["dist"]) == int(out["distance"].sum()), i
        seen_edits += s["n_edits"]
    assert seen_edits > 100


def test_generated_inputs_ran_and_met_every_shape(lines):
    gen = [rec for name, _, rec in lines if name == "gen"]
    assert len(gen) == 8 and all(int(rec["rc"]) == 0 for rec in gen)
    assert int(gen[0]["valid"]) == -1 and int(gen[0]["canonical"]) == -1  # no threads
    assert int(gen[1]["valid"]) == 1  # one thread
    assert any(int(rec["edits"]) > 50 for rec in gen) and any(int(rec["classes"]) > 5 for rec in gen)
    assert all(int(rec["edits"]) == int(rec["dist"]) for rec in gen)  # every script whole, none above the cap


def test_refusals(lines):
    refused = {name: int(rec["rc"]) for name, _, rec in lines if name in ("twice", "past", "negative", "long", "flags")}
    assert refused == {"twice": -22, "past": -22, "negative": -22, "long": -22, "flags": -22}
