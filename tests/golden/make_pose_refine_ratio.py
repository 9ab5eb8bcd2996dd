"""The ratio r that tests/test_gpu_pose.py::test_refine_pose_recovers_a_known_offset records: refine_pose's loop run in
float64 on the CPU (oracle/gsplat_oracle.py render, oracle/train_oracle.py loss, tests/pose_oracle.py six sums and Adam
retraction) on a reduced copy of the test's case - a quarter of the Gaussians on a quarter of the pixels at the same field
of view - with the test's offset, rates and step count.  Prints the final / initial pose error (angle, translation).

    python tests/golden/make_pose_refine_ratio.py        # about five seconds
"""
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

import pose_cases as PC  # noqa: E402

if __name__ == "__main__":
    model, cam, distance = PC.refine_scene(PC.REFINE_N // 4, (PC.REFINE_DIMS[0] // 2, PC.REFINE_DIMS[1] // 2))
    rows = []
    ratios = PC.oracle_refine(model, cam, distance, report=lambda step, loss, err: rows.append((step, loss, *err)))
    for step, loss, angle, shift in rows[::10] + rows[-1:]:
        print(f"step {step:3d}  loss {loss:.5f}  angle {angle:.6f} rad  translation {shift:.6f}")
    print(f"steps {PC.REFINE_STEPS}, lr_translation {PC.REFINE_LR_T}, lr_rotation {PC.REFINE_LR_R}: "
          f"final / initial error: angle {ratios[0]:.4f}, translation {ratios[1]:.4f}")
