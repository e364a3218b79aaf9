"""Records tests/golden/model_ops.json: for every handle of tests/model_ops.py the op list (name, kernel, arithmetic, flops, bytes,
launches), memory_bytes(), the feature map's side and the layer table.  tests/test_model_ops.py holds every later build to it: which
kernel runs an op, and in which weight format, is decided when the graph is built, and a refactor of that decision changes nothing
here.

Needs no GPU (rpn_model_create touches no device; without one the CU count reads 256, the MI355X's).  Record from the build whose
choices are the contract -- the commit BEFORE a change to model.hip -- by pointing RPN_HIP_LIB at that build's library:
    RPN_HIP_LIB=/path/to/parent/librpn_hip.so python tests/golden/make_model_ops.py [output.json]
Every op and layer string is stored once, in "strings"; a handle lists indices into it."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import model_ops as mo  # noqa: E402
from tf_rpn_amd import _lib as L  # noqa: E402


def main(path):
    strings, index, handles = [], {}, {}

    def intern(s):
        if s not in index:
            index[s] = len(strings)
            strings.append(s)
        return index[s]

    for h in mo.HANDLES:
        r = mo.record_of(h)
        r["ops"] = [intern(s) for s in r["ops"]]
        r["layers"] = [intern(s) for s in r["layers"]]
        handles[mo.key_of(h)] = r
    with open(path, "w") as f:
        f.write('{"cu_count": %d,\n"strings": [\n' % mo.CU_COUNT + ",\n".join(json.dumps(s) for s in strings) + '\n],\n"handles": {\n'
                + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(handles[k], sort_keys=True, separators=(",", ":")))
                             for k in sorted(handles)) + "\n}}\n")
    print("wrote %d handles, %d strings from %s to %s" % (len(handles), len(strings), L.LIB_PATH, path))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "model_ops.json"))
