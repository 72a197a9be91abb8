"""csrc/workspace.h, the carver that lays the side checkers' device arrays out
in one arena: tests/workspace_main.cpp built with g++ and the address and
undefined-behaviour sanitizers, run as a child process.  The program lays out
about 30 arrays in the append driver's shape (a full call, then one whose
per-mop and per-read arrays are empty), fills every array and reads it back;
its lines say where each array landed in the sizing and the binding pass."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def layouts(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed"
    exe = str(tmp_path_factory.mktemp("workspace") / "workspace_main")
    # the sanitizers' runtimes linked in statically: the program needs no place in anybody's preload list
    subprocess.check_call([cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           os.path.join(HERE, "workspace_main.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    out = []
    for block in r.stdout.split("next\n"):
        rows, total = [], None
        for line in block.splitlines():
            f = line.split()
            if f[0] == "total":
                total = (int(f[1]), int(f[2]))
            else:
                rows.append(dict(name=f[0], count=int(f[1]), elem=int(f[2]), sized=int(f[3]), bound=int(f[4]),
                                 null_when_sizing=bool(int(f[5]))))
        out.append((rows, total))
    assert len(out) == 2
    return out


def test_shape(layouts):
    (full, _), (bare, _) = layouts
    assert len(full) == len(bare) >= 29
    assert all(r["count"] > 0 for r in full)
    assert sum(r["count"] == 0 for r in bare) >= 10


@pytest.mark.parametrize("which", (0, 1), ids=("full", "empty arrays"))
def test_passes_agree(layouts, which):
    rows, total = layouts[which]
    assert total[0] == total[1] > 0
    assert [r["sized"] for r in rows] == [r["bound"] for r in rows]
    assert all(r["null_when_sizing"] for r in rows)


@pytest.mark.parametrize("which", (0, 1), ids=("full", "empty arrays"))
def test_aligned_disjoint_inside(layouts, which):
    rows, (total, _) = layouts[which]
    assert total % 256 == 0
    spans = sorted((r["bound"], r["bound"] + max(r["count"] * r["elem"], 256), r["name"]) for r in rows)
    for a, b, name in spans:
        assert a % 256 == 0 and 0 <= a < b <= total, (name, a, b, total)
    for (_, b, n0), (a, _, n1) in zip(spans, spans[1:]):
        assert b <= a, (n0, n1)
    # no more than the rounding between two arrays: the sizes are ensure()'s
    assert total == sum((max(r["count"] * r["elem"], 256) + 255) // 256 * 256 for r in rows)


def test_empty_array_has_256_bytes_of_its_own(layouts):
    rows, (total, _) = layouts[1]
    starts = sorted(r["bound"] for r in rows) + [total]
    for r in rows:
        if r["count"] == 0:
            nxt = starts[starts.index(r["bound"]) + 1]
            assert nxt - r["bound"] == 256, r["name"]  # (a null pointer would have failed the program's fill)
