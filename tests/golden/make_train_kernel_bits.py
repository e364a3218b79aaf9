"""Records tests/golden/train_kernel_bits.json: the SHA-256 of every output of the training path's backward kernels on the seeded,
real-valued cases of tests/train_bits.py, through the public single-layer entries.  tests/test_gpu_train_bits.py holds every later
build to these digests: the order of each sum is part of the library's contract ("the same bits on every run").

Needs a GPU.  Record from the build whose bits are the contract -- the commit BEFORE a change to these kernels -- by pointing
RPN_HIP_LIB at that build's library:
    RPN_HIP_LIB=/path/to/parent/librpn_hip.so python tests/golden/make_train_kernel_bits.py [output.json]
A case whose two runs disagree is not written (and the recorder exits non-zero); neither is anything when an input builder fails
the order-sensitivity check (integer-valued inputs would: their sums are exact in any order)."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import train_bits as tb  # noqa: E402
from tf_rpn_amd import _lib as L  # noqa: E402


def main(path):
    for name, (build_a, build_b) in tb.BUILDER_PAIRS.items():
        if not tb.order_sensitive(build_a, build_b):
            sys.exit("%s: two summation orders give the same float32 bits -- digests of such inputs pin nothing" % name)
    L.require_gpu()
    lib = L.lib()
    records, bad = [], []
    for entry, shape in tb.CASES:
        seed = tb.seed_of(entry, shape)
        first, second = tb.digests(lib, entry, shape, seed), tb.digests(lib, entry, shape, seed)
        for output in sorted(first):
            if first[output] != second[output]:
                bad.append((entry, shape, output))
                continue
            records.append({"entry": entry, "output": output, "shape": list(shape), "seed": seed, "sha256": first[output]})
            print("%-28s %-4s %-24s seed %7d  %s" % (entry, output, tuple(shape), seed, first[output]))
    if bad:
        sys.exit("two runs of the same case disagree, nothing written: %s" % bad)
    with open(path, "w") as f:
        f.write("[\n" + ",\n".join(" " + json.dumps(r, sort_keys=True) for r in records) + "\n]\n")
    print("wrote %d digests from %s to %s" % (len(records), L.LIB_PATH, path))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "train_kernel_bits.json"))
