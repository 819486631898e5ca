"""Generate tests/golden/reference_sweep.npz: a random sweep of compute_hamming_dist and binaryToInt through the
REFERENCE's own code (oracle/_ref/libvcref.so), so that test_oracle_cpu.py::test_primitives_against_live_reference
checks the oracle against the reference's outputs on every machine, not only where the reference is mounted.

Run in the authoring container only (the reference does not travel):
    make -C oracle ref && python tests/golden/make_reference_sweep.py
The output is data only: inputs (uint8 rows) and the reference's outputs.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import vc_oracle as vo  # noqa: E402

R = vo.ref()
assert R is not None, "build oracle/_ref first (make -C oracle ref)"
rng = np.random.default_rng(1)
out = {}
for nb in (8, 16, 32, 64, 13):
    a = rng.integers(0, 256, (300, nb), dtype=np.uint8)
    b = rng.integers(0, 256, (300, nb), dtype=np.uint8)
    out["ham_a_%d" % nb], out["ham_b_%d" % nb] = a, b
    out["ham_d_%d" % nb] = np.array([R.vcref_hamming(x.tobytes(), y.tobytes(), nb) for x, y in zip(a, b)], dtype=np.int32)
for ln in (1, 2, 3, 4):
    p = rng.integers(0, 256, (500, ln), dtype=np.uint8)
    out["b2i_in_%d" % ln] = p
    out["b2i_out_%d" % ln] = np.array([R.vcref_binary_to_int(x.tobytes(), ln) for x in p], dtype=np.uint32)

path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_sweep.npz")
np.savez_compressed(path, **out)
print(path, os.path.getsize(path))
