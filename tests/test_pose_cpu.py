"""Camera pose refinement on the host: the identity behind ts_pose_grad against plain autograd
through the float64 oracle, the g++ build of csrc/pose_math.h against the numpy restatement, SE(3)'s Exp and Log, the
retraction, and PoseModel's host state.  No GPU needed."""
import copy

import numpy as np
import pytest
import torch

import pose_cases as PC
import pose_oracle as PO
from tinysplat_amd import pose
from tinysplat_amd.synthetic import quat_to_rot_matrix


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return PC.build_host(tmp_path_factory.mktemp("pose"))


# ---- 1. the identity
def test_six_sums_of_the_oracles_rows_are_autograds_pose_gradient():
    """60 Gaussians, 48 x 32, degree 0, raw quaternions of norm ~1.7 |randn|, a rotated and translated camera from a
    normalised quaternion, weighted RGB + depth loss, all float64: the six sums over the oracle's own means.grad and
    quats.grad equal the gradient autograd gives the view matrix, within 1e-10 of the largest component (float64
    rounding over ~1e3 operations with four orders of margin; measured 1.4e-16)."""
    scene, view, ref = PC.small_scene_reference()
    assert ref["clamped"].sum() >= 1, "no Gaussian beyond the fov clamp reaches the image"
    assert ref["culled"].sum() >= 1, "no Gaussian is culled"
    assert np.abs(ref["v_means"][ref["clamped"]]).max() > 0
    got = PO.pose_gradient(view, scene["means"], scene["quats"], ref["v_means"], ref["v_quats"])
    scale = np.abs(ref["pose"]).max()
    err = np.abs(got - ref["pose"]).max()
    print(f"largest component {scale:.6g}, largest difference {err:.3g} ({err / scale:.3g} relative)")
    assert scale > 1.0 and err <= 1e-10 * scale


def test_identity_needs_an_orthonormal_rotation():
    """The condition, documented: with R built from a quaternion of norm 1.02 without normalising it
    (synthetic.quat_to_rot_matrix) the six sums miss autograd's gradient by more than 1e-5 relative (measured 7e-4)."""
    scene, _view, _ref = PC.small_scene_reference()
    view = np.eye(4)
    view[:3, :3] = quat_to_rot_matrix(1.02 * np.array([0.97, 0.06, -0.12, 0.09]))
    view[:3, 3] = -view[:3, :3] @ np.array([0.3, -0.2, -0.5])
    assert np.abs(view[:3, :3].T @ view[:3, :3] - np.eye(3)).max() > 1e-4
    ref = PC.oracle_pose_run(scene, view)
    got = PO.pose_gradient(view, scene["means"], scene["quats"], ref["v_means"], ref["v_quats"])
    assert np.abs(got - ref["pose"]).max() > 1e-5 * np.abs(ref["pose"]).max()


# ---- 2. the host build
@pytest.mark.parametrize("n,zero", [(n, z) for n in PC.SIZES for z in ("none", "ends")] + [(PC.MANY, "none")])
def test_host_build_matches_the_numpy_restatement(host, n, zero):
    rows = PC.random_rows(n, seed=100 + n, zero=zero)
    view = PC.view_matrix().astype(np.float32)
    got = PC.host_pose_grad(host, view, *rows)
    want = PO.pose_gradient(view, *rows)
    bound = PC.rounding_bound(view, *rows)
    if n == 0:
        assert np.array_equal(got, np.zeros(6)) and not np.signbit(got).any()
        return
    ratio = np.abs(got - want) / np.maximum(bound, np.finfo(np.float64).tiny)
    print(f"n = {n}, {zero}: worst error / bound {ratio.max():.3g}")
    assert (np.abs(got - want) <= bound).all()
    assert np.abs(want).max() > 0 or (zero == "ends" and n <= 9)       # (every row of a tiny case is an end row)


def test_host_build_sums_zero_rows_to_positive_zero(host):
    rows = PC.random_rows(4097, seed=3, zero="all")
    got = PC.host_pose_grad(host, PC.view_matrix(), *rows)
    assert np.array_equal(got, np.zeros(6)) and not np.signbit(got).any()


def test_host_build_row_terms(host):
    """One row against the definition, component by component (the translation part is R g, the rotation part
    p x R g + R tau)."""
    m, q, g, h = (a[0] for a in PC.random_rows(1, seed=11))
    view = np.ascontiguousarray(PC.view_matrix()[:3, :], dtype=np.float32)
    out = np.zeros(6)
    host.ph_pose_row(PC._f(view), PC._f(m), PC._f(q), PC._f(g), PC._f(h), out.ctypes.data_as(PC.F64P))
    want = PO.row_terms(view, m[None], q[None], g[None], h[None])[0]
    assert np.allclose(out, want, rtol=0, atol=1e-13 * np.abs(want).max())


# ---- 3. Exp, Log, the retraction
ANGLES = (0.0, 1e-12, 1e-4, 1.0, np.pi - 1e-3)


@pytest.mark.parametrize("theta", ANGLES)
def test_exp_log_round_trip_and_series(theta):
    axis = np.array([0.36, -0.48, 0.8])
    delta = np.concatenate([[0.4, -1.2, 2.0], theta * axis])
    T = pose.se3_exp(delta)
    assert np.abs(T[:3, :3].T @ T[:3, :3] - np.eye(3)).max() < 4e-16 and T[3].tolist() == [0, 0, 0, 1]
    back = pose.se3_log(T)
    # Log divides by sin-like factors that shrink towards pi: 1e-3 from it the rotation vector keeps ~1e-13
    assert np.abs(back - delta).max() <= (1e-12 if theta > 3 else 1e-14) * max(1.0, np.abs(delta).max())
    try:
        from scipy.linalg import expm
        want = expm(PO.twist(delta))
    except ImportError:
        want = PO.se3_exp(delta)
    assert np.abs(T - want).max() <= 1e-14 * max(1.0, np.abs(want).max())
    assert np.abs(T - PO.se3_exp(delta)).max() <= 1e-13 * max(1.0, np.abs(want).max())


def test_log_of_exp_of_small_translations_is_exact_at_zero_rotation():
    d = np.array([1.0, 2.0, -3.0, 0.0, 0.0, 0.0])
    assert np.array_equal(pose.se3_log(pose.se3_exp(d)), d)
    assert np.array_equal(pose.se3_exp(np.zeros(6)), np.eye(4))


def test_retraction_keeps_the_quaternion_unit_and_matches_the_matrix_product():
    g = np.random.default_rng(0)
    q, t = np.array([1.0, 0.0, 0.0, 0.0]), np.zeros(3)
    T = np.eye(4)
    for k in range(10_000):
        d = 1e-2 * g.normal(size=6)
        q, t = pose.retract(q, t, d)
        if k < 200:
            T = PO.se3_exp(d) @ T
            if k == 199:
                Tq = np.eye(4)
                Tq[:3, :3], Tq[:3, 3] = PC.quat_to_rot(q), t
                assert np.abs(Tq - T).max() < 1e-12
    assert abs(np.linalg.norm(q) - 1.0) <= 2.0 ** -52


def test_adam_retraction_update_matches_the_oracle():
    cam = PC.camera_from_view(PC.view_matrix(), 48, 32)
    cfg = pose.PoseConfig(lr_translation=3e-3, lr_rotation=2e-3, weight_decay=1e-2)
    pm = pose.PoseModel([cam], cfg)
    g = np.random.default_rng(1)
    T, m, v = np.eye(4), np.zeros(6), np.zeros(6)
    for step in range(1, 6):
        grad = g.normal(size=6) * 100.0
        pm.step(0, grad)
        T, m, v = PO.adam_retraction(T, m, v, step, grad, [3e-3] * 3 + [2e-3] * 3, cfg.betas, cfg.eps, cfg.weight_decay,
                                     pose.se3_log)
        assert np.abs(pm.correction(0) - T).max() < 1e-13
    assert np.allclose(pm.exp_avg[0], m, rtol=1e-14, atol=0) and np.allclose(pm.exp_avg_sq[0], v, rtol=1e-14, atol=0)
    angle, shift = pm.corrections()[0]
    want = PO.pose_error(np.eye(4), T)
    assert abs(angle - want[0]) < 1e-12 and abs(shift - want[1]) < 1e-12


# ---- 4. PoseModel
def test_config_defaults_are_the_documented_ones():
    c = pose.PoseConfig()
    assert (c.lr_translation, c.lr_rotation, c.weight_decay, c.betas, c.eps) == (1e-5, 1e-5, 1e-6, (0.9, 0.999), 1e-15)
    with pytest.raises(ValueError):
        pose.PoseConfig(lr_rotation=-1.0)


def test_identity_correction_keeps_the_cameras_bits_and_zero_gradient_moves_nothing():
    cams = [PC.camera_from_view(PC.view_matrix(), 48, 32),
            PC.camera_from_view(PC.view_matrix((0.5, -0.5, 0.4, 0.6), (1.0, 2.0, -3.0)), 48, 32)]
    pm = pose.PoseModel(cams, pose.PoseConfig(weight_decay=0.0))
    for i, c in enumerate(cams):
        held = pm.camera(i)
        assert held is not c and held is pm.camera(i) and held.f_x == c.f_x and held.proj_matrix is c.proj_matrix
        assert held.view_matrix.dtype == torch.float32 and torch.equal(held.view_matrix, c.view_matrix)
        before = held.view_matrix
        pm.step(i, np.zeros(6))
        assert pm.camera(i) is held and held.view_matrix is not before            # a fresh tensor on the same object
        assert torch.equal(held.view_matrix, before)
    assert pm.steps == [1, 1] and np.array_equal(pm.corrections(), np.zeros((2, 2)))
    # zero rates: any gradient leaves the matrix bits alone (the moments still move)
    still = pose.PoseModel(cams, pose.PoseConfig(lr_translation=0.0, lr_rotation=0.0, weight_decay=0.0))
    still.step(1, np.array([3.0, -2.0, 1.0, 0.5, 0.25, -8.0]))
    assert torch.equal(still.camera(1).view_matrix, cams[1].view_matrix) and still.exp_avg[1].any()
    assert torch.equal(cams[1].view_matrix, PC.camera_from_view(PC.view_matrix((0.5, -0.5, 0.4, 0.6), (1.0, 2.0, -3.0)),
                                                                48, 32).view_matrix)   # the base camera is not touched


def test_a_sloppy_rotation_is_projected_once():
    view = np.eye(4)
    view[:3, :3] = quat_to_rot_matrix(1.02 * np.array([0.97, 0.06, -0.12, 0.09]))
    pm = pose.PoseModel([PC.camera_from_view(view, 48, 32)])
    R = pm.base[0][:3, :3]
    assert np.abs(R.T @ R - np.eye(3)).max() < 4e-15 and np.linalg.det(R) > 0
    # the polar factor is the nearest rotation in the Frobenius norm: nearer than the quaternion's own rotation
    sloppy = np.asarray(view[:3, :3], dtype=np.float32).astype(np.float64)
    assert np.linalg.norm(R - sloppy) <= np.linalg.norm(PC.quat_to_rot((0.97, 0.06, -0.12, 0.09)) - sloppy) < 1e-2


def test_state_dict_round_trip(tmp_path):
    cams = [PC.camera_from_view(PC.view_matrix(), 48, 32), PC.camera_from_view(PC.view_matrix(position=(1, 1, 1)), 48, 32)]
    pm = pose.PoseModel(cams, pose.PoseConfig(lr_translation=1e-3, lr_rotation=2e-3))
    g = np.random.default_rng(2)
    for k in range(5):
        pm.step(k % 2, g.normal(size=6))
    pm.save(tmp_path / "poses.pth")
    back = pose.PoseModel.load(tmp_path / "poses.pth", cams)
    assert back.config == pm.config and back.steps == pm.steps
    for name in ("quats", "trans", "exp_avg", "exp_avg_sq", "base"):
        assert np.array_equal(getattr(back, name), getattr(pm, name)), name
    for a, b in zip(back.cameras(), pm.cameras()):
        assert torch.equal(a.view_matrix, b.view_matrix)
    grad = g.normal(size=6)
    assert np.array_equal(back.step(1, grad), copy.deepcopy(pm).step(1, grad))
    with pytest.raises(ValueError):
        pose.PoseModel(cams[:1]).load_state_dict(pm.state_dict())
    with pytest.raises(IndexError):
        pm.camera(2)
    # corrections are refused on cameras they were not trained on: the saved base matrices are compared
    with pytest.raises(ValueError, match="other cameras"):
        pose.PoseModel.load(tmp_path / "poses.pth", cams[::-1])
    moved = PC.camera_from_view(PC.view_matrix(position=(1, 1, 1.001)), 48, 32)
    with pytest.raises(ValueError, match="view 1"):
        pose.PoseModel.load(tmp_path / "poses.pth", [cams[0], moved])
