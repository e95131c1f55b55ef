"""The BatchNorm family's workspace contract, pinned on the CPU.

Every BN entry point sizes its chunk partials with bn_geo (csrc/bn_act.hip): the callers allocate what
rgan_bn_partial_bytes / rgan_bn_dd_partial_bytes answer, and the kernels write [chunks][NS][C]
doubles into it.  The library loads without a GPU, so this test compares both functions' answers
with tests/golden/bn_partial_bytes.json for pixel counts around every chunking threshold and
channel counts on and off the vector path, plus the "no such layer" arguments, which answer 0.

A refactor of the BN code (a split of bn_act.hip into units, say) leaves the fixture alone.  A deliberate change of the chunking
regenerates it (``python -m tests.test_bn_geometry_cpu --write``) and shows the diff in review.
"""
import json
import os
import sys

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bn_partial_bytes.json")

PS = (1, 15, 16, 17, 511, 512, 513, 1023, 1024, 1025, 2048, 2049, 66563, 131072, 2097152)
CS = (1, 3, 4, 6, 8, 16, 20, 64, 70, 128, 256, 512, 1024, 2048)
EMPTY = ((0, 64), (-1, 64), (512, 0))  # (P, C) that name no layer


def record():
    """{"P,C": [rgan_bn_partial_bytes, rgan_bn_dd_partial_bytes]}"""
    from relativisticgan_amd import _lib
    lib = _lib.lib()
    pairs = [(P, C) for P in PS for C in CS] + list(EMPTY)
    return {f"{P},{C}": [int(lib.rgan_bn_partial_bytes(P, C)), int(lib.rgan_bn_dd_partial_bytes(P, C))]
            for P, C in pairs}


def _dump(rows):
    return "{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(v)}" for k, v in rows.items()) + "\n}\n"


def write_fixture():
    with open(FIXTURE, "w") as f:
        f.write(_dump(record()))


def test_partial_bytes_match_fixture():
    """Both size queries of every (P, C) equal the recorded ones; P <= 0 or C <= 0 answers 0."""
    with open(FIXTURE) as f:
        want = json.load(f)
    got = record()
    assert list(got) == list(want)
    assert len(got) == len(PS) * len(CS) + len(EMPTY)
    bad = {k: (got[k], want[k]) for k in got if got[k] != want[k]}
    assert not bad, bad
    for P, C in EMPTY:
        assert got[f"{P},{C}"] == [0, 0]


if __name__ == "__main__":
    if sys.argv[1:] == ["--write"]:
        write_fixture()
    else:
        sys.exit("usage: python -m tests.test_bn_geometry_cpu --write")
