"""The batches of tests/test_gpu_record_transpose.py without a GPU: the CPU
oracle's JITC verdict and fail op of every key equal the plant's construction
(batch() asserts it), every length, deciding record and line alignment the
GPU test names is present, and every invalid key has its valid twin."""
import numpy as np

import test_gpu_record_transpose as T


def test_oracle_equals_the_construction():
    for name in T.GROUPS:
        pls, ops, off, j = T.batch(name)
        assert len(pls) == len(j) and (np.diff(off) == [len(pl.recs) for pl in pls]).all()
        assert (j["verdict"] == 0).any() and (j["verdict"] == 1).any()
    T.test_every_invalid_key_has_its_valid_twin()


def test_every_named_edge_is_present():
    pls, _, off, j = T.batch("lengths")
    for n in T.LENGTHS:
        assert {int(v) for v, k in zip(j["verdict"], np.diff(off)) if k == n} == {0, 1}, n
    pls, _, off, j = T.batch("records")
    assert (np.diff(off) == 1024).all()
    assert set(T.RECORDS) <= {int(f) for f in j["fail_op"]}
    pls, _, off, j = T.batch("aligned")
    for a in range(8):
        at = [k for k in range(len(pls)) if off[k] % 8 == a and len(pls[k].recs) > 8]
        assert {int(j["verdict"][k]) for k in at} == {0, 1}, a
