"""csrc/perfstats_host.cpp: tests/perfstats_main.cpp built with g++ and the
address and undefined-behaviour sanitizers, run as a child process (as
tests/test_watch_host_sanitize.py runs its program).  The program checks the
KATs' arrays and inputs this test generates, then inputs of its own, every
array sized exactly; its lines carry each call's counts, which must be those
the library gives through the binding."""
import json
import os
import random
import shutil
import struct
import subprocess

import numpy as np
import pytest

from jepsen.etcd_amd import abi
from test_perfstats import events_of, random_history

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "jepsen", "etcd_amd", "csrc")
KATS = json.load(open(os.path.join(HERE, "golden", "perfstats_kat.json")))["cases"]
FIELDS = (("valid", "valid"), ("client", "n_client"), ("pairs", "n_pairs"), ("pending", "n_pending"),
          ("ignored", "n_ignored_completions"), ("mismatched", "n_mismatched_f"), ("count", "count"), ("ok", "ok"),
          ("fail", "fail"), ("info", "info"), ("tmax", "t_max"), ("nrate", "n_rate_buckets"),
          ("nquant", "n_quant_buckets"))
M = 1000003


def c_mod(a, m):
    """C's a % m for numpy int64 arrays (the sign of the dividend)."""
    return np.sign(a) * (np.abs(a) % m)


def inputs():
    """The KATs, then generated histories: (events, n_f, qs, rate_dt, quant_dt)."""
    out = [(events_of(k["events"]), k["n_f"], k["qs"], k["rate_dt"], k["quant_dt"]) for k in KATS]
    rng = random.Random(0x5A17)
    for i in range(40):
        n_f = rng.randint(1, 9)
        rows = random_history(rng, rng.randrange(0, 1500), rng.randint(1, 20), n_f, rng.choice((0.0, 0.1)), 1000)
        out.append((events_of(rows), n_f, [0.5, 0.95, 0.99, 1.0][:i % 5], rng.choice((5000, 10000)),
                    rng.choice((9999, 30000))))
    return out


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed"
    tmp = tmp_path_factory.mktemp("perfstats")
    exe, cases = str(tmp / "perfstats_main"), str(tmp / "cases.bin")
    ins = inputs()
    with open(cases, "wb") as f:
        f.write(struct.pack("<q", len(ins)))
        for ev, n_f, qs, rate_dt, quant_dt in ins:
            f.write(struct.pack("<qii8dqq", len(ev), n_f, len(qs), *(list(qs) + [0.0] * (8 - len(qs))), rate_dt,
                                quant_dt))
            f.write(np.ascontiguousarray(ev, dtype=abi.PS_EVENT_DTYPE).tobytes())
    # the sanitizers' runtimes linked in statically: the program needs no place in anybody's preload list
    subprocess.check_call([cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", CSRC,
                           os.path.join(HERE, "perfstats_main.cpp"), os.path.join(CSRC, "perfstats_host.cpp"),
                           "-o", exe])
    env = {k: v for k, v in os.environ.items() if not k.startswith("LC_PS_")}
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
    seen_pairs = 0
    for i, ((ev, n_f, qs, rate_dt, quant_dt), rec) in enumerate(zip(ins, cases)):
        out, s = abi.perf_stats_host(ev, n_f, qs, rate_dt, quant_dt)
        assert int(rec["rc"]) == 0, i
        assert [int(rec[a]) for a, _ in FIELDS] == [s[b] for _, b in FIELDS], (i, rec, s)
        q = out["quant"][out["quant"] != abi.LC_PS_NONE]
        assert int(rec["quantsum"]) == int(c_mod(q, M).sum()), i
        if i % 2 == 0:  # (the program asked for the point arrays)
            paired = out["comp_pos"] >= 0
            assert int(rec["paired"]) == int(paired.sum()) == s["n_pairs"], i
            assert int(rec["latsum"]) == int(c_mod(out["latency_ns"][paired], M).sum()), i
        seen_pairs += s["n_pairs"]
    assert seen_pairs > 1000


def test_generated_inputs_ran_and_met_every_shape(lines):
    gen = [rec for name, _, rec in lines if name == "gen"]
    assert len(gen) == 6 and all(int(rec["rc"]) == 0 for rec in gen)
    assert int(gen[0]["client"]) == 0 and int(gen[0]["valid"]) == 1  # no events
    assert int(gen[1]["client"]) == 383 and int(gen[1]["pairs"]) > 20  # one process
    assert int(gen[2]["pairs"]) == 0 and int(gen[2]["pending"]) + int(gen[2]["ignored"]) == 716  # all their own
    assert all(int(rec["pairs"]) == int(rec["paired"]) for rec in gen[:5]) and int(gen[5]["paired"]) == 0
    assert all(int(rec["count"]) == int(rec["ok"]) + int(rec["fail"]) + int(rec["info"]) for rec in gen)


def test_refusals(lines):
    names = ("time", "type", "f", "nf", "nq", "dt", "q", "maxf", "table")
    refused = {name: int(rec["rc"]) for name, _, rec in lines if name in names}
    assert refused == {"time": -22, "type": -22, "f": -22, "nf": -22, "nq": -22, "dt": -22, "q": -22, "maxf": -7,
                       "table": -7}
