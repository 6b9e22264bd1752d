"""The start state of tests/test_gpu_quat_stages.py (its docstring tells the rows and the conditioning bound), in a plain module so
that tests/test_gpu_model_constants.py starts its steady role-split cells from the same poses."""
import numpy as np
from scipy.spatial.transform import Rotation

import workspace_poses as wp

KAPPA_MAX = 1.5e4  # largest condition number of J^T J a drawn start pose may have (the docstring of tests/test_gpu_quat_stages.py)
REST, TURNING = 0, 1
TURN_RATE = 200.0  # rad/s: 0.2 rad in the 1 ms of world step 0


_start = {}


def td_condition(st, pose7):
    """Condition number of J^T J at a pose (fp64, the oracle's structure matrix)."""
    import oracle

    jac = oracle.ik(st, np.asarray(pose7, dtype=np.float64))[3]
    return float(np.linalg.cond(jac.T @ jac))


def start_state(pkg, n, batch):
    """(pose7, twist6) float32 of the docstring of tests/test_gpu_quat_stages.py, and the largest kappa of the batch."""
    if (n, batch) not in _start:
        model = wp.cell_model(pkg, n)
        st = pkg.Config(model=model, batch=1, stages=3).to_struct()
        rng = np.random.default_rng(1000 * n + batch)
        pose = np.tile(np.asarray(model.home_pose(), dtype=np.float64), (batch, 1))
        box, drawn = [], 0
        while len(box) < batch - 10:
            for p in wp.box_poses(model, batch - 10, rng, "W"):
                drawn += 1
                if len(box) < batch - 10 and td_condition(st, p.astype(np.float32)) <= KAPPA_MAX:
                    box.append(p)
            assert drawn <= 20 * batch, "box W of this model holds hardly any well-conditioned pose"
        pose[2:batch - 8] = box
        axes = np.vstack([np.eye(3), np.ones((1, 3)) / np.sqrt(3.0)])
        pose[batch - 8:, 3:] = Rotation.from_rotvec(np.concatenate([0.3 * axes, -0.3 * axes])).as_quat()
        twist = np.zeros((batch, 6))
        twist[TURNING, 3:] = TURN_RATE / np.sqrt(3.0)
        pose = pose.astype(np.float32)
        _start[(n, batch)] = (pose, twist.astype(np.float32), max(td_condition(st, p) for p in pose))
    return _start[(n, batch)]
