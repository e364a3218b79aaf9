"""Records tests/golden/forward_bits.json: the SHA-256 of `reg | cls` (float32 bytes) of every forward of the cases of
tests/forward_bits.py, of the activations they read back, and the status flags the forwards raised.
tests/test_gpu_forward_bits.py holds every later build to these digests.

Needs a GPU.  Record from the build whose bits are the contract -- the commit BEFORE a change to the forward -- by pointing
RPN_HIP_LIB at that build's library:
    RPN_HIP_LIB=/path/to/parent/librpn_hip.so python tests/golden/make_forward_bits.py [output.json]
Every case runs twice, each time on a fresh handle; if two runs of any case disagree nothing is written (and the recorder exits
non-zero)."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import forward_bits as fb  # noqa: E402
from tf_rpn_amd import _lib as L  # noqa: E402


def main(path):
    L.require_gpu()
    records, bad = [], []
    for case in fb.CASES:
        first, second = fb.run_case(case), fb.run_case(case)
        if first != second:
            bad.append(fb.key_of(case))
            continue
        records.append({"case": fb.key_of(case), "sha256": first[0], "status": first[1]})
        print("%-36s status %d  %s" % (fb.key_of(case), first[1], " ".join("%s=%s" % (k, v[:12]) for k, v in sorted(first[0].items()))),
              flush=True)
    if bad:
        sys.exit("two runs of the same case disagree, nothing written: %s" % bad)
    with open(path, "w") as f:
        f.write("[\n" + ",\n".join(" " + json.dumps(r, sort_keys=True) for r in records) + "\n]\n")
    print("wrote %d cases from %s to %s" % (len(records), L.LIB_PATH, path))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "forward_bits.json"))
