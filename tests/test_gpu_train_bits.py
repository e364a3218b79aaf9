"""The bits of the training path's backward kernels, pinned: every output of every case of tests/train_bits.py has the SHA-256
that tests/golden/train_kernel_bits.json records (tests/golden/make_train_kernel_bits.py; recorded once, from the build before
the kernels' shared pieces were merged).  The inputs are real-valued, so a reordered sum changes a digest; the integer bit-exact
tests, the float64 parity tests and the determinism tests would all let one through.  A digest that changes on purpose is
re-recorded with the recorder, from the build that is to become the contract."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import __graft_entry__ as entry_points  # noqa: E402
import train_bits as tb  # noqa: E402
from tf_rpn_amd import _lib as L  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "train_kernel_bits.json")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        entry_points.build()
    return L.lib()


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN) as f:
        return {(r["entry"], tuple(r["shape"]), r["output"]): r for r in json.load(f)}


OUTPUTS = {"rpn_conv3x3_wgrad": ("db", "dw"), "rpn_conv3x3_wgrad_wide": ("db", "dw"), "rpn_dwconv3x3_dgrad": ("dx",),
           "rpn_dwconv3x3_s2_dgrad": ("dx",)}


def test_every_case_is_recorded_once(recorded):
    """A case is recorded or it is not in the table: the file holds exactly the table's cases, each output once, at the table's seed."""
    want = {(e, s, o) for e, s in tb.CASES for o in OUTPUTS.get(e, ("dw",))}
    assert set(recorded) == want
    with open(GOLDEN) as f:
        assert len(json.load(f)) == len(want)
    for (e, s, _o), r in recorded.items():
        assert r["seed"] == tb.seed_of(e, s), (e, s)
        assert len(r["sha256"]) == 64


@pytest.mark.parametrize("pair", sorted(tb.BUILDER_PAIRS))
def test_inputs_make_the_digest_order_sensitive(pair):
    """Two orders of the same float32 sum of products differ for every pair of input builders -- and do not for integers."""
    assert tb.order_sensitive(*tb.BUILDER_PAIRS[pair])

    def ints(rng, shape):
        return rng.randint(-3, 4, size=shape).astype("float32")
    assert not tb.order_sensitive(ints, ints)


@pytest.mark.gpu
@pytest.mark.parametrize("entry,shape", tb.CASES)
def test_kernel_bits_match_the_record(lib, recorded, entry, shape):
    got = tb.digests(lib, entry, shape, tb.seed_of(entry, shape))
    assert sorted(got) == sorted(OUTPUTS.get(entry, ("dw",)))
    for output, sha in sorted(got.items()):
        assert sha == recorded[(entry, shape, output)]["sha256"], (entry, shape, output)
