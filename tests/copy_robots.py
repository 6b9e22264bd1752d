"""What tests/test_copy_robots_inputs.py (CPU) and tests/test_gpu_copy_robots.py (GPU) share: the test map of cdpr_copy_robots, the
pure-Python statement of what a valid map is, and the "twin from birth" inputs - the input rows of every destination replaced by those
of its source, so that an oracle started on them holds, at every step, what a copied engine must hold after the copy."""
import numpy as np

import robot_histories as ri

B = ri.B


def destinations_of(source):
    s = np.asarray(source, dtype=np.int64)
    return (s >= 0) & (s != np.arange(len(s)))


def validate_map(source, batch=None):
    """None where cdpr_copy_robots accepts the map, else (robot, why) of the first entry it refuses: a destination's source must be a
    robot of the batch and must itself be left as it is."""
    s = np.asarray(source, dtype=np.int64)
    batch = len(s) if batch is None else batch
    dest = destinations_of(s)
    for r in np.flatnonzero(dest):
        if s[r] >= batch:
            return int(r), "out of range"
        if dest[s[r]]:
            return int(r), "chain"
    return None


def copy_map(batch=B):
    """Destinations: reset_mask()'s robots (every fourth plus 0, 63, 64, 129).  Sources: outside that mask, in another `index mod 3`
    group than their destination (the mode changes).  Robot 2 feeds both 0 and 4; every other destination d starts looking at d + 65,
    so most sources sit in another wavefront than their destination."""
    mask = ri.reset_mask(batch).astype(bool)
    source = np.full(batch, -1, dtype=np.int32)
    for d in np.flatnonzero(mask):
        if d in (0, 4):
            source[d] = 2
            continue
        s = (d + 65) % batch
        while mask[s] or s % 3 == d % 3:
            s = (s + 1) % batch
        source[d] = s
    return source


def aligned_map(batch=B):
    """Robots 64 .. 127 take robots 0 .. 63: whole wavefronts, lane for lane."""
    source = np.full(batch, -1, dtype=np.int32)
    source[64:128] = np.arange(64)
    return source


def twin_rows(inputs, source):
    """`inputs` (history_inputs / after_inputs: arrays with one row per robot) with every destination's row replaced by its source's."""
    dest = destinations_of(source)
    out = {}
    for k, v in inputs.items():
        v = np.array(v, copy=True)
        v[dest] = v[np.asarray(source)[dest]]
        out[k] = v
    return out
