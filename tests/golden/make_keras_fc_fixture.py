"""keras_vgg16_fc_tiny.h5: the tail of a Keras VGG16 in miniature (block5_conv3, flatten, fc1, fc2, predictions), written by the
REAL h5py / libhdf5 the way make_h5_fixtures.py writes its files; pins DetectionHead.load_keras_weights.

Run with the interpreter that has h5py (the one make_h5_fixtures.py names):
    /opt/conda/bin/python3.9 tests/golden/make_keras_fc_fixture.py
fc1 is (2 * 2 * 4, 8): a head of pooling_size (2, 2), channels 4, hidden (8, 8).  Every array's contents are
make_h5_fixtures.expected_array of its path, so the tests need no companion file."""
import os

from make_h5_fixtures import HERE, write

VGG_FC_TINY = [   # (layer, [(weight, shape)])
    ("block5_conv3", [("kernel", (3, 3, 4, 4)), ("bias", (4,))]),
    ("flatten", []),
    ("fc1", [("kernel", (16, 8)), ("bias", (8,))]),
    ("fc2", [("kernel", (8, 8)), ("bias", (8,))]),
    ("predictions", [("kernel", (8, 10)), ("bias", (10,))]),
]

if __name__ == "__main__":
    path = os.path.join(HERE, "keras_vgg16_fc_tiny.h5")
    write(path, VGG_FC_TINY, strings="vlen")
    print(os.path.basename(path), os.path.getsize(path))
