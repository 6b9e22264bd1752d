"""A numpy decoder of a recorded observable image, written from DESIGN.md section 3 alone: it owes nothing to the library, so a getter
that equals it is checked against the layout and not against another path through the same code.

fp32 handles: rows of float4 slots, float32[slots][stride][4]
    image  0: px py pz qx | 1: qy qz qw vx | 2: vy vz wx wy | 3: wz fk_residual fk_iterations flags | 4 ..: q, q', effort, ceil(n / 4) slots each
precision = 64 handles: rows of doubles, float64[rows][stride]
    image  0 - 6 pose | 7 - 12 twist | 13 fk_residual | 14 fk_iterations | 15 flags | 16 ..: q, q', effort, n rows each
stride = bytes of the buffer / bytes of one row of it over all slots (rows); robots [0, B) are real, the rest is padding.
"""
import numpy as np


def image_rows(n, fp64):
    """float4 slots (fp32) or double rows (precision = 64) of one observable image"""
    return 16 + 3 * n if fp64 else 4 + 3 * ((n + 3) // 4)


def _platform(buf, B, fp64):
    """pose7, twist6 out of rows shaped [rows][stride] (doubles) or [slots][stride][4] (floats)"""
    if fp64:
        return buf[0:7, :B].T.copy(), buf[7:13, :B].T.copy()
    flat = np.concatenate([buf[s, :B, :] for s in range(4)], axis=1)  # [B][16]: slots 0 - 3 side by side
    return flat[:, 0:7].copy(), flat[:, 7:13].copy()


def decode_image(raw, B, n, fp64):
    """One observable image (uint8) -> dict of position, velocity, effort [B, n], pose [B, 7], twist [B, 6], fk_residual, fk_iterations,
    flags [B], in the image's own number type."""
    rows = image_rows(n, fp64)
    raw = np.ascontiguousarray(raw, dtype=np.uint8)
    if fp64:
        stride = raw.size // (rows * 8)
        buf = raw.view(np.float64).reshape(rows, stride)
        joint = [buf[16 + f * n:16 + (f + 1) * n, :B].T.copy() for f in range(3)]
        extra = [buf[13 + k, :B].copy() for k in range(3)]
    else:
        stride = raw.size // (rows * 16)
        buf = raw.view(np.float32).reshape(rows, stride, 4)
        G = (n + 3) // 4
        joint = [np.concatenate([buf[4 + f * G + g, :B, :] for g in range(G)], axis=1)[:, :n].copy() for f in range(3)]
        extra = [buf[3, :B, 1 + k].copy() for k in range(3)]
    pose, twist = _platform(buf, B, fp64)
    return dict(position=joint[0], velocity=joint[1], effort=joint[2], pose=pose, twist=twist, fk_residual=extra[0], fk_iterations=extra[1], flags=extra[2])


def hand_built_image(B, n, fp64, stride):
    """An image written element by element from the layout's address rule, every element a number that names its column and its robot
    (exact in float32): (raw uint8, what decode_image must return).  Padding columns hold -1."""
    tag = lambda col, r: float(col * 1024 + r)  # noqa: E731
    names = [("position", n), ("velocity", n), ("effort", n), ("pose", 7), ("twist", 6), ("fk_residual", 1), ("fk_iterations", 1), ("flags", 1)]
    want, col0 = {}, {}
    c = 0
    for name, w in names:
        col0[name] = c
        a = np.array([[tag(c + j, r) for j in range(w)] for r in range(B)])
        want[name] = a if name in ("position", "velocity", "effort", "pose", "twist") else a[:, 0]
        c += w
    rows = image_rows(n, fp64)
    if fp64:
        flat = np.full(rows * stride, -1.0, dtype=np.float64)
        where = lambda row, r: row * stride + r  # noqa: E731
        for r in range(B):
            for j in range(7):
                flat[where(j, r)] = tag(col0["pose"] + j, r)
            for j in range(6):
                flat[where(7 + j, r)] = tag(col0["twist"] + j, r)
            for k, name in enumerate(("fk_residual", "fk_iterations", "flags")):
                flat[where(13 + k, r)] = tag(col0[name], r)
            for f, name in enumerate(("position", "velocity", "effort")):
                for i in range(n):
                    flat[where(16 + f * n + i, r)] = tag(col0[name] + i, r)
    else:
        flat = np.full(rows * stride * 4, -1.0, dtype=np.float32)
        where = lambda slot, comp, r: (slot * stride + r) * 4 + comp  # noqa: E731
        G = (n + 3) // 4
        for r in range(B):
            for j in range(7):  # px py pz qx | qy qz qw .
                flat[where(j // 4, j % 4, r)] = tag(col0["pose"] + j, r)
            for j in range(6):  # . . . vx | vy vz wx wy | wz
                flat[where((7 + j) // 4, (7 + j) % 4, r)] = tag(col0["twist"] + j, r)
            for k, name in enumerate(("fk_residual", "fk_iterations", "flags")):
                flat[where(3, 1 + k, r)] = tag(col0[name], r)
            for f, name in enumerate(("position", "velocity", "effort")):
                for i in range(n):
                    flat[where(4 + f * G + i // 4, i % 4, r)] = tag(col0[name] + i, r)
    want = {k: v.astype(flat.dtype) for k, v in want.items()}
    return flat.view(np.uint8), want

