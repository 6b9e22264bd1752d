"""The read-out's reference, checked without a GPU: tests/readout_layout.py decodes an observable image written element by element
from the address rule of DESIGN.md section 3 (every element names its column and its robot), at the cable counts where the number of
float4 slots per joint field changes (n = 4, 8, 12) and one past each (5, 9; 1 below the first).  The library's own decoders
(cdpr_decode_observables*) need a handle and so a GPU: tests/test_gpu_readout.py compares them with this decoder."""
import numpy as np
import pytest

import readout_layout as rl


@pytest.mark.parametrize("fp64", (False, True), ids=("fp32", "fp64"))
@pytest.mark.parametrize("n", (1, 4, 5, 8, 9, 12))
def test_decoder_reads_a_hand_built_image(n, fp64):
    B, stride = 67, 128  # a ragged batch inside two wavefronts of padding
    raw, want = rl.hand_built_image(B, n, fp64, stride)
    assert raw.size == rl.image_rows(n, fp64) * stride * (8 if fp64 else 16)
    got = rl.decode_image(raw, B, n, fp64)
    assert set(got) == set(want)
    seen = []
    for name, w in want.items():
        g = got[name]
        assert g.dtype == (np.float64 if fp64 else np.float32) and g.shape == w.shape, name
        assert np.array_equal(g, w), name
        seen.append(g.ravel())
    seen = np.concatenate(seen)
    assert seen.size == B * (3 * n + 16) and np.unique(seen).size == seen.size  # every column of every robot, each once, no padding
