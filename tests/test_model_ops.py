"""What rpn_model_create decides, pinned: every handle of tests/model_ops.py has the op list (name, kernel, arithmetic, flops, bytes,
launches), the memory_bytes(), the feature map side and the layer table that tests/golden/model_ops.json records
(tests/golden/make_model_ops.py; recorded from the build before the kernel choice moved into one function).  No device is touched:
the test runs wherever the library loads.  A choice that changes on purpose is re-recorded with the recorder."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import __graft_entry__ as entry_points  # noqa: E402
import model_ops as mo  # noqa: E402
from tf_rpn_amd import _lib as L  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "model_ops.json")


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN) as f:
        data = json.load(f)
    strings = data["strings"]
    out = {}
    for key, r in data["handles"].items():
        out[key] = dict(r, ops=[strings[i] for i in r["ops"]], layers=[strings[i] for i in r["layers"]])
    return data["cu_count"], out


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        entry_points.build()
    return L.lib()


def device_cu_count():
    """The compute units of device 0, or None without a device (the library then assumes 256)."""
    import torch
    if not torch.cuda.is_available():
        return None
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def test_the_file_holds_exactly_the_tables_handles(recorded):
    cu, handles = recorded
    assert cu == mo.CU_COUNT
    assert len(mo.HANDLES) == 144 and len({mo.key_of(h) for h in mo.HANDLES}) == 144
    assert set(handles) == {mo.key_of(h) for h in mo.HANDLES}
    assert os.path.getsize(GOLDEN) < 200 * 1000


@pytest.mark.parametrize("handle", mo.HANDLES, ids=mo.key_of)
def test_handle_matches_the_record(lib, recorded, handle):
    cu = device_cu_count()
    if cu is not None and cu != mo.CU_COUNT:
        pytest.skip("the record is for %d compute units, this device has %d" % (mo.CU_COUNT, cu))
    got, want = mo.record_of(handle), recorded[1][mo.key_of(handle)]
    assert got["ops"] == want["ops"]
    assert got["memory_bytes"] == want["memory_bytes"]
    assert got["feature_map_shape"] == want["feature_map_shape"]
    assert got["layers"] == want["layers"]
