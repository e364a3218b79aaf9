#!/bin/bash
# Build the -DRPN_STAMP variant next to the product library (tf_rpn_amd/csrc/librpn_hip_stamp.so), then restore the product build.
# The stamps are in the 16x16x32 split conv kernels (conv_split16_kernels.hip).
set -eo pipefail
cd "$(dirname "$0")/../tf_rpn_amd/csrc"
quiet() { grep -E "error|warning" || true; }          # (grep finding nothing is not a failure; make failing is: pipefail)
make EXTRA_conv_split16_kernels="-DRPN_STAMP $1" -B _build/conv_split16_kernels.o librpn_hip.so 2>&1 | quiet
cp librpn_hip.so librpn_hip_stamp.so
make -B _build/conv_split16_kernels.o librpn_hip.so 2>&1 | quiet
