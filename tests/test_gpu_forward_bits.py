"""The bits of the forward, pinned: every forward of every case of tests/forward_bits.py gives the SHA-256 of `reg | cls` that
tests/golden/forward_bits.json records (tests/golden/make_forward_bits.py; recorded on the MI355X from the build before each op's
kernel was chosen in one place), the activations read back afterwards give theirs, and rpn_model_status reads the recorded flags.
A route that packs its weights for one kernel and launches another, or a launch sequence that changed, changes a digest; the parity
tests against the float64 oracle allow 1e-4 and would let a reordered sum through.  A digest that changes on purpose is re-recorded
with the recorder, from the build that is to become the contract."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import __graft_entry__ as entry_points  # noqa: E402
import forward_bits as fb  # noqa: E402
from tf_rpn_amd import _lib as L  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "forward_bits.json")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        entry_points.build()
    return L.lib()


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN) as f:
        return {r["case"]: r for r in json.load(f)}


def test_every_case_is_recorded_once(recorded):
    """The file holds exactly the table's cases, and for each exactly the digests the case yields."""
    assert len(fb.CASES) == 24 and set(recorded) == {fb.key_of(c) for c in fb.CASES}
    with open(GOLDEN) as f:
        assert len(json.load(f)) == len(fb.CASES)
    for case in fb.CASES:
        r = recorded[fb.key_of(case)]
        assert sorted(r["sha256"]) == sorted(fb.outputs_of(case)), fb.key_of(case)
        assert all(len(v) == 64 for v in r["sha256"].values())
        assert isinstance(r["status"], int)


def test_the_inputs_are_real_valued():
    """Seeded images in [0, 1) and He-normal weights: their float32 sums depend on the order they are taken in."""
    imgs = fb.images_of(96, 2)
    assert imgs.dtype.name == "float32" and imgs.min() >= 0.0 and imgs.max() < 1.0 and (imgs != imgs.round()).all()


@pytest.mark.gpu
@pytest.mark.parametrize("case", fb.CASES, ids=fb.key_of)
def test_forward_bits_match_the_record(lib, recorded, case):
    got, status = fb.run_case(case)
    want = recorded[fb.key_of(case)]
    assert sorted(got) == sorted(fb.outputs_of(case))
    for name in fb.outputs_of(case):
        assert got[name] == want["sha256"][name], (fb.key_of(case), name)
    assert status == want["status"], fb.key_of(case)
