"""Scene editing without a GPU: the SH rotation matrices against the oracle's basis, the Sim3
algebra, the orientation from cameras, the camera move, the host build of csrc/transform_math.h against the float64
oracle of tests/transform_oracle.py under the sequential-sum bounds, the render invariance through the CPU oracle, the
merge, the C entries' argument errors and the export tool's new flags."""
import ctypes
import importlib.util
import math
from pathlib import Path

import numpy as np
import pytest
import torch

import transform_cases as TC
import transform_oracle as TO
from helpers import oracle_frame, scene_args
from tinysplat_amd import edit
from tinysplat_amd.edit import Sim3, sh_rotation_matrices
from tinysplat_amd.synthetic import PinholeCamera, SplatModel

ROOT = Path(__file__).resolve().parent.parent
ROT_A = TO.quat_to_matrix(TC.QUAT)
ROT_B = TO.quat_to_matrix((0.9, 0.1, -0.4, 0.6))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return TC.build_host(tmp_path_factory.mktemp("transform"))


# ------------------------------------------------------------------------------------------------ D_l
def test_fit_directions_are_well_conditioned():
    for l in range(1, 5):
        d = edit._fit_directions(l)
        assert d.shape == (2 * l + 1, 3) and np.allclose(np.linalg.norm(d, axis=1), 1.0, atol=1e-15)
        assert np.linalg.cond(edit.sh_band(l, d)) <= 1e3


def test_module_basis_is_the_oracles():
    d = TO.random_directions(50, 3)
    ref = TO.basis(4, d)
    for l in range(1, 5):
        assert np.array_equal(edit.sh_band(l, d), ref[:, l * l:(l + 1) ** 2])


@pytest.mark.parametrize("rot", [ROT_A, ROT_B, ROT_B @ ROT_A], ids=["a", "b", "ba"])
def test_defining_identity_on_random_directions(rot):
    """sum_j Y_lj(d) D_l[j, k] = Y_lk(R^T d) on 1000 random directions against the oracle's sh_basis in float64."""
    d = TO.random_directions(1000, 5)
    mats = sh_rotation_matrices(rot, 4)
    b, a = TO.basis(4, d), TO.basis(4, d @ rot)
    for l, dl in enumerate(mats, start=1):
        cols = slice(l * l, (l + 1) ** 2)
        err = np.abs(b[:, cols] @ dl - a[:, cols]).max()
        print(f"degree {l}: identity to {err:.2e}")
        assert err <= 1e-12
        assert np.abs(dl @ dl.T - np.eye(2 * l + 1)).max() <= 1e-12
        assert np.abs(dl - TO.sh_rotation(rot, 4)[l - 1]).max() <= 1e-12        # the oracle's least-squares route


def test_sh_rotation_is_a_representation_and_exact_at_the_identity():
    ba, a, b = (sh_rotation_matrices(r, 4) for r in (ROT_B @ ROT_A, ROT_A, ROT_B))
    for l in range(4):
        assert np.abs(ba[l] - b[l] @ a[l]).max() <= 1e-12
    for l, m in enumerate(sh_rotation_matrices(np.eye(3), 4), start=1):
        assert np.array_equal(m, np.eye(2 * l + 1))
    assert sh_rotation_matrices(ROT_A, 0) == [] and len(sh_rotation_matrices(ROT_A, 2)) == 2
    with pytest.raises(ValueError):
        sh_rotation_matrices(ROT_A, 5)
    with pytest.raises(ValueError):
        sh_rotation_matrices(np.eye(4), 2)


def test_quarter_turn_about_z_permutes_band_one_with_signs():
    """R^T d = (d_y, -d_x, d_z) and band 1 is (-C1 y, C1 z, -C1 x): Y_0(R^T d) = C1 d_x = -Y_2(d) and Y_2(R^T d) = -C1 d_y =
    Y_0(d), so c'_0 = c_2, c'_1 = c_1 and c'_2 = -c_0."""
    t = Sim3.from_quat((math.sqrt(0.5), 0.0, 0.0, math.sqrt(0.5)))
    assert np.abs(t.rotation - np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]])).max() < 1e-15
    d1 = sh_rotation_matrices(t.rotation, 1)[0]
    assert np.abs(d1 - np.array([[0.0, 0, 1], [0, 1, 0], [-1, 0, 0]])).max() <= 1e-15


# ------------------------------------------------------------------------------------------------ Sim3
def test_sim3_algebra():
    a, b = Sim3.from_quat(TC.QUAT, TC.TRANSLATION, 2.5), Sim3.from_quat((0.9, 0.1, -0.4, 0.6), (-3.0, 0.25, 1.0), 0.4)
    pts = np.random.default_rng(0).normal(size=(20, 3))
    assert np.abs(a.apply(pts) - (2.5 * pts @ ROT_A.T + np.array(TC.TRANSLATION))).max() < 1e-14
    assert np.abs(a.inverse().apply(a.apply(pts)) - pts).max() < 1e-14
    assert np.abs((a @ b).apply(pts) - a.apply(b.apply(pts))).max() < 1e-14
    assert np.abs((a @ a.inverse()).matrix() - np.eye(4)).max() < 1e-15
    assert np.array_equal(Sim3.identity().matrix(), np.eye(4))
    back = Sim3.from_matrix(a.matrix())
    assert np.abs(back.rotation - a.rotation).max() < 1e-15 and abs(back.scale - 2.5) < 1e-15
    assert np.array_equal(back.translation, a.translation)
    assert np.abs(TO.quat_to_matrix(a.quat()) - a.rotation).max() < 1e-15 and abs(np.linalg.norm(a.quat()) - 1) < 1e-15
    for q in ((0.0, 1, 0, 0), (0.0, 0, 1, 0), (0.0, 0, 0, 1), (1e-3, 0.6, -0.8, 0.0), (-0.5, 0.5, 0.5, -0.5)):
        s = Sim3.from_quat(q)                                    # every branch of the matrix -> quaternion conversion
        assert np.abs(TO.quat_to_matrix(s.quat()) - s.rotation).max() < 1e-15
    for s3 in (a, b, Sim3.from_quat((-0.2, 0.9, 0.1, 0.3))):          # a rotation's and its inverse's quaternions are conjugates
        assert s3.quat()[0] >= 0 and np.abs(s3.inverse().quat() - s3.quat() * [1, -1, -1, -1]).max() < 1e-15
    with pytest.raises(Exception):
        a.scale = 2.0                                            # frozen
    with pytest.raises(ValueError):
        a.rotation[0, 0] = 2.0                                   # and so are its arrays
    # a float32 view matrix passes the relative check, also at a scale far from 1
    cam = PinholeCamera.look_at_origin_plus_z(64, 48, position=(1.0, 2.0, 3.0), quat=np.array(TC.QUAT) / np.linalg.norm(TC.QUAT))
    v = Sim3.from_matrix(cam.view_matrix)
    assert abs(v.scale - 1.0) < 1e-6 and np.abs(v.rotation - ROT_A).max() < 1e-6
    big = a.matrix().astype(np.float32) * np.float32(1000.0)
    big[3] = (0, 0, 0, 1)
    assert abs(Sim3.from_matrix(big).scale - 2500.0) < 1e-3


def test_sim3_rejections():
    good = Sim3.from_quat(TC.QUAT, TC.TRANSLATION, 2.5).matrix()
    last_row = good.copy()
    last_row[3, 0] = 1e-3
    shear = good.copy()
    shear[0, 1] += 1e-4 * 2.5
    stretch = good.copy()
    stretch[:3, 0] *= 1.001
    mirror = good.copy()
    mirror[:3, :3] = mirror[:3, :3] @ np.diag([1.0, 1.0, -1.0])
    singular = good.copy()
    singular[:3, :3] = 0.0
    nan = good.copy()
    nan[0, 3] = np.nan
    for bad in (last_row, shear, stretch, mirror, singular, nan, good[:3]):
        with pytest.raises(ValueError):
            Sim3.from_matrix(bad)
    for kw in (dict(scale=0.0), dict(scale=-1.0), dict(scale=float("inf")), dict(translation=(0.0, np.nan, 0.0))):
        with pytest.raises(ValueError):
            Sim3.from_quat(TC.QUAT, **kw)
    with pytest.raises(ValueError):
        Sim3.from_quat((0.0, 0.0, 0.0, 0.0))
    with pytest.raises(ValueError):
        Sim3(np.diag([1.0, 1.0, -1.0]), np.zeros(3), 1.0)
    with pytest.raises(ValueError):
        Sim3(np.eye(3) + 1e-4, np.zeros(3), 1.0)


# ------------------------------------------------------------------------------------------------ cameras
def _ring(up, centre, radius, count=12, tilt=0.3):
    """Cameras on a circle of `radius` about `centre` in the plane normal to `up`, looking at the axis from slightly
    above; their image y axes average to -up.  Built with ``update_view_matrix``, which stores float32; the float64 matrix
    of the same pose is then put in its place, since the checks below ask for 1e-12."""
    up = np.asarray(up, dtype=np.float64) / np.linalg.norm(up)
    e1 = np.cross(up, [1.0, 0.0, 0.0] if abs(up[0]) < 0.9 else [0.0, 1.0, 0.0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(up, e1)
    cams = []
    for i in range(count):
        phi = 2 * math.pi * i / count
        out = math.cos(phi) * e1 + math.sin(phi) * e2
        pos = np.asarray(centre, dtype=np.float64) + radius * out
        z = -math.cos(tilt) * out - math.sin(tilt) * up          # looking inwards and down
        x = np.cross(z, up)
        x /= np.linalg.norm(x)
        y = np.cross(z, x)                                       # image y: down
        rot = np.stack([x, y, z])                                # world -> camera rows
        cam = PinholeCamera.look_at_origin_plus_z(64, 48)
        cam.update_view_matrix(pos, edit._matrix_to_quat(rot))
        v = np.eye(4)
        v[:3, :3], v[:3, 3] = rot, -rot @ pos
        cam.view_matrix = torch.as_tensor(v, dtype=torch.float64)             # float64: the 1e-12 of the check
        cams.append(cam)
    return cams


def test_update_view_matrix_builds_the_rings_cameras():
    """The ring's float64 view matrices are what ``update_view_matrix`` stores in float32."""
    cam = _ring((0.0, 1.0, 0.0), (1.0, 2.0, 3.0), 2.0)[3]
    ref = PinholeCamera.look_at_origin_plus_z(64, 48)
    v = cam.view_matrix.numpy()
    ref.update_view_matrix(-v[:3, :3].T @ v[:3, 3], edit._matrix_to_quat(v[:3, :3]))
    assert np.abs(ref.view_matrix.numpy() - v).max() < 1e-6


@pytest.mark.parametrize("up", [(0.0, -1.0, 0.0), (0.3, 0.5, -0.8), (0.0, 0.0, 1.0)])
def test_orient_from_cameras_recovers_up_centre_and_radius(up):
    centre, radius = np.array([4.0, -2.0, 7.0]), 3.5
    cams = _ring(up, centre, radius)
    t = edit.orient_from_cameras(cams)
    u = np.asarray(up) / np.linalg.norm(up)
    assert np.abs(t.rotation @ u - np.array([0.0, 0.0, 1.0])).max() <= 1e-12
    assert np.abs(t.apply(centre)).max() <= 1e-12 and abs(t.scale - 1.0 / radius) <= 1e-12
    moved = edit.transform_cameras(cams, t)
    centres = np.stack([-(c.view_matrix.numpy()[:3, :3].T @ c.view_matrix.numpy()[:3, 3]) for c in moved])
    assert np.abs(np.linalg.norm(centres, axis=1) - 1.0).max() < 1e-6 and np.abs(centres[:, 2]).max() < 1e-6
    # the minimal rotation leaves the axis u x up alone
    axis = np.cross(u, [0.0, 0.0, 1.0])
    if np.linalg.norm(axis) > 1e-9:
        assert np.abs(t.rotation @ axis - axis).max() <= 1e-12
    plain = edit.orient_from_cameras(cams, center=False, unit_scale=False)
    assert plain.scale == 1.0 and np.array_equal(plain.translation, np.zeros(3))
    other = edit.orient_from_cameras(cams, up=(0.0, 1.0, 0.0))
    assert np.abs(other.rotation @ u - np.array([0.0, 1.0, 0.0])).max() <= 1e-12


def test_orient_half_turn_and_degenerate_rules():
    down = _ring((0.0, 0.0, -1.0), (0.0, 0.0, 0.0), 1.0)         # world up is exactly -z
    t = edit.orient_from_cameras(down)
    # up = +z: the smallest |up_a| is a = 0 (ties to the lowest index), the axis normalise(z x e_x) = +y
    assert np.abs(t.rotation - np.diag([-1.0, 1.0, -1.0])).max() <= 1e-12
    t = edit.orient_from_cameras(_ring((-1.0, 0.0, 0.0), (0.0, 0.0, 0.0), 1.0), up=(1.0, 0.0, 0.0))
    # up = +x: a = 1, the axis normalise(x x e_y) = +z
    assert np.abs(t.rotation - np.diag([-1.0, -1.0, 1.0])).max() <= 1e-12
    # two cameras whose up directions cancel: no rotation; one camera: no scale
    a, b = _ring((0.0, 1.0, 0.0), (0.0, 0.0, 0.0), 1.0, count=1, tilt=0.0), _ring((0.0, -1.0, 0.0), (1.0, 0.0, 0.0), 1.0, count=1, tilt=0.0)
    t = edit.orient_from_cameras(a + b)
    assert np.array_equal(t.rotation, np.eye(3)) and t.scale > 0
    one = edit.orient_from_cameras(a)
    assert one.scale == 1.0 and np.abs(one.rotation @ np.array([0.0, 1.0, 0.0]) - np.array([0.0, 0.0, 1.0])).max() <= 1e-12
    with pytest.raises(ValueError):
        edit.orient_from_cameras([])
    with pytest.raises(ValueError):
        edit.orient_from_cameras(a, up=(0.0, 0.0, 0.0))


def test_transform_camera_scales_camera_space():
    """V' x' = s V x in float64 on random points, by the module's formula and by the oracle's 4x4 product."""
    cam = _ring((0.2, 0.9, 0.1), (1.0, 2.0, 3.0), 4.0)[5]
    v = cam.view_matrix.numpy()
    pts = np.random.default_rng(2).normal(size=(100, 3)) * 5
    for s in TC.SCALES:
        t = TC.sim3(s)
        rot = v[:3, :3] @ t.rotation.T
        vp = np.eye(4)
        vp[:3, :3], vp[:3, 3] = rot, s * v[:3, 3] - rot @ t.translation          # what transform_camera builds, in float64
        assert np.abs(vp - TO.camera_view(v, s, t.rotation, t.translation)).max() <= 1e-12
        lhs = t.apply(pts) @ vp[:3, :3].T + vp[:3, 3]
        assert np.abs(lhs - s * (pts @ v[:3, :3].T + v[:3, 3])).max() <= 1e-12
        new = edit.transform_camera(cam, t)
        assert new.view_matrix.dtype == torch.float32 and new is not cam and cam.view_matrix.dtype == torch.float64
        assert np.abs(new.view_matrix.numpy() - vp).max() <= 1e-6 * max(1.0, np.abs(vp).max())
        assert new.proj_matrix is cam.proj_matrix and (new.f_x, new.f_y, new.width, new.height, new.fov_x, new.fov_y) == \
            (cam.f_x, cam.f_y, cam.width, cam.height, cam.fov_x, cam.fov_y)
    pts32 = torch.as_tensor(pts, dtype=torch.float32)
    moved = edit.transform_points(pts32, TC.sim3(2.5))
    assert moved.dtype == torch.float32 and np.abs(moved.numpy() - TC.sim3(2.5).apply(pts)).max() < 1e-5
    assert np.abs(edit.transform_points(torch.as_tensor(pts), TC.sim3(0.4)).numpy() - TC.sim3(0.4).apply(pts)).max() < 1e-14


# ------------------------------------------------------------------------------------------------ the host build
@pytest.mark.parametrize("degree", [0, 1, 2, 3, 4])
def test_host_build_is_within_the_bounds_of_the_oracle(host, degree):
    scene = TC.with_edges(4000 if degree == 3 else 300, degree, seed=degree)
    for s in (2.5, 0.4):
        xform, quat, log_scale, sh, mats = TC.arguments(TC.sim3(s), degree)
        got = TC.host_transform(host, scene, xform, quat, log_scale, sh)
        worst = TC.check_against_oracle(got, scene, xform, quat, log_scale, mats)
        print(f"degree {degree}, s = {s}: worst error / bound {worst}")


def test_host_build_of_the_edge_scene_alone(host):
    scene = TC.edge_scene(3)
    xform, quat, log_scale, sh, mats = TC.arguments(TC.sim3(2.5), 3)
    got = TC.host_transform(host, scene, xform, quat, log_scale, sh)
    TC.check_against_oracle(got, scene, xform, quat, log_scale, mats)
    assert np.isnan(got["quats"][1]).all() and np.array_equal(got["quats"][0], np.zeros(4, np.float32))
    assert not got["rest"][:6].any()                              # rows whose SH are zero stay zero


def test_identity_returns_its_input(host):
    scene = TC.with_edges(300, 3, seed=8)
    xform, quat, log_scale, sh, _ = TC.arguments(Sim3.identity(), 3)
    assert np.array_equal(xform, np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32)) and log_scale == 0.0
    assert np.array_equal(quat, np.array([1, 0, 0, 0], np.float32))
    got = TC.host_transform(host, scene, xform, quat, log_scale, sh)
    for f in TC.FIELDS:
        finite = np.isfinite(got[f])
        assert np.array_equal(got[f][finite], scene[f][finite]), f             # == : the sign of a zero may differ
        assert np.array_equal(np.isfinite(scene[f].reshape(len(scene[f]), -1)).all(1),
                              finite.reshape(len(scene[f]), -1).all(1)), f      # 0 * inf spoils only rows that hold one


def test_mask_copies_rows_and_known_answer(host):
    scene = TC.with_edges(300, 2, seed=4)
    xform, quat, log_scale, sh, _ = TC.arguments(TC.sim3(2.5), 2)
    mask = np.random.default_rng(1).random(300) < 0.5
    full = TC.host_transform(host, scene, xform, quat, log_scale, sh)
    part = TC.host_transform(host, scene, xform, quat, log_scale, sh, mask)
    for f in TC.FIELDS:
        assert np.array_equal(TC.bits(part[f][~mask]), TC.bits(scene[f][~mask])), f
        assert np.array_equal(TC.bits(part[f][mask]), TC.bits(full[f][mask])), f
    # a quarter turn about z, twice the size, moved by (1, 2, 3), one Gaussian of degree 1, written out
    t = Sim3.from_quat((math.sqrt(0.5), 0.0, 0.0, math.sqrt(0.5)), (1.0, 2.0, 3.0), 2.0)
    xform, quat, log_scale, sh, _ = TC.arguments(t, 1)
    one = {"means": np.array([[1.0, 10.0, 100.0]], np.float32), "scales": np.array([[0.0, -1.0, 0.5]], np.float32),
           "quats": np.array([[2.0, 0.0, 0.0, 0.0]], np.float32),
           "rest": np.array([[[1.0, 2.0, 3.0], [10.0, 20.0, 30.0], [100.0, 200.0, 300.0]]], np.float32)}
    got = TC.host_transform(host, one, xform, quat, log_scale, sh)
    assert np.allclose(got["means"], [[-19.0, 4.0, 203.0]], rtol=0, atol=1e-5)
    assert np.array_equal(got["scales"], one["scales"] + np.float32(math.log(2.0)))
    assert np.allclose(got["quats"], [[math.sqrt(2.0), 0.0, 0.0, math.sqrt(2.0)]], rtol=0, atol=1e-6)
    assert np.allclose(got["rest"], [[[100.0, 200.0, 300.0], [10.0, 20.0, 30.0], [-1.0, -2.0, -3.0]]], rtol=0, atol=1e-4)
    assert TC.host_transform(host, TC.random_scene(5, 0, 0), xform, quat, log_scale, sh[:0])["rest"].shape == (5, 0, 3)


def test_host_box_mask(host):
    means = np.array([[0.0, 0, 0], [1.0, 2, 3], [1.0, 2, 3.0000002], [-1.0, -2, -3], [np.nan, 0, 0], [0.5, np.inf, 0],
                      [1.0000001, 0, 0]], np.float32)
    box = np.concatenate([np.diag(1.0 / np.array([1.0, 2.0, 3.0])).reshape(-1), np.zeros(3)]).astype(np.float32)
    got = TC.host_box_mask(host, box, means)
    with np.errstate(all="ignore"):
        v = ((box[:9].reshape(3, 3)[None, :, 0] * means[:, None, 0] + box[:9].reshape(3, 3)[None, :, 1] * means[:, None, 1])
             + box[:9].reshape(3, 3)[None, :, 2] * means[:, None, 2]) + box[9:][None, :]
    assert v.dtype == np.float32 and np.array_equal(got, (np.abs(v) <= 1).all(1))
    assert got[[0, 1, 3]].all() and not got[[4, 5, 6]].any()      # the centre and two corners; NaN, Inf, one ulp outside


# ------------------------------------------------------------------------------------------------ render invariance
def _moved_on_the_host(model, cam, t):
    """The module's host path: ``sh_rotation_matrices`` and the float64 definition, rounded to float32."""
    degree = model.active_sh_degree
    mats = sh_rotation_matrices(t.rotation, degree)
    xform = np.concatenate([(t.scale * t.rotation).reshape(-1), t.translation])
    ref = TO.transform(xform, t.quat(), math.log(t.scale), mats, model.means.numpy(), model.scales.numpy(),
                       model.quats.numpy(), model.colors_rest.numpy())
    f32 = lambda a: torch.from_numpy(a.astype(np.float32))
    moved = SplatModel(f32(ref["means"]), model.colors_dc, f32(ref["rest"]), f32(ref["scales"]), f32(ref["quats"]),
                       model.opacities, active_sh_degree=degree, background=model.background)
    return moved, edit.transform_camera(cam, t)


@pytest.fixture(scope="module")
def reference_render():
    model, cam = scene_args(400, 3, 64, 48, seed=3, scale_mult=4.0)
    with torch.no_grad():
        return model, cam, oracle_frame(model, cam, (64, 48), correct_viewdirs=True)


@pytest.mark.parametrize("s", TC.SCALES)
def test_oracle_render_is_invariant(reference_render, s):
    """rgb to 1e-3 and depth' = s depth to 1e-3 max(1, s) with correct_viewdirs=True: a condition of the definition (the
    oracle with an independent float64 transform measured 2e-5 and 1e-4), which unrotated SH miss by 0.39."""
    model, cam, ref = reference_render
    t = TC.sim3(s)
    moved, moved_cam = _moved_on_the_host(model, cam, t)
    with torch.no_grad():
        out = oracle_frame(moved, moved_cam, (64, 48), correct_viewdirs=True)
        rgb = (out["rgb"] - ref["rgb"]).abs().max().item()
        depth = (out["depth"] - s * ref["depth"]).abs().max().item()
        plain = SplatModel(moved.means, moved.colors_dc, model.colors_rest, moved.scales, moved.quats, moved.opacities,
                           active_sh_degree=3, background=model.background)
        unrotated = (oracle_frame(plain, moved_cam, (64, 48), depth=False, correct_viewdirs=True)["rgb"] - ref["rgb"]).abs().max().item()
    print(f"s = {s}: rgb {rgb:.2e}, depth {depth:.2e}, with the SH left unrotated {unrotated:.2f}")
    assert rgb <= 1e-3 and depth <= 1e-3 * max(1.0, s)
    assert unrotated > 0.05                                       # the scene is sensitive to the SH rotation


# ------------------------------------------------------------------------------------------------ merge, C entries, tools
def test_merge_models():
    a, _ = scene_args(5, 0, 16, 16, seed=1)
    b, _ = scene_args(7, 2, 16, 16, seed=2)
    c, _ = scene_args(3, 3, 16, 16, seed=3)
    a.background = torch.tensor([0.1, 0.2, 0.3])
    m = edit.merge_models([a, b, c])
    assert m.num_points == 15 and m.colors_rest.shape == (15, 15, 3) and m.active_sh_degree == 3
    assert m.background is a.background
    for f in ("means", "colors_dc", "scales", "quats", "opacities"):
        assert torch.equal(getattr(m, f), torch.cat([getattr(x, f) for x in (a, b, c)]))
    assert not m.colors_rest[:5].any() and torch.equal(m.colors_rest[5:12, :8], b.colors_rest)
    assert not m.colors_rest[5:12, 8:].any() and torch.equal(m.colors_rest[12:], c.colors_rest)
    single = edit.merge_models([b])
    assert torch.equal(single.colors_rest, b.colors_rest) and single.active_sh_degree == 2
    with pytest.raises(ValueError):
        edit.merge_models([])
    meta = SplatModel(*[p.to("meta") for p in b.parameters()], active_sh_degree=2)
    with pytest.raises(ValueError, match="devices"):
        edit.merge_models([a, meta])


def test_entries_report_argument_errors_without_a_gpu():
    from tinysplat_amd import _lib
    lib = _lib.load()
    f4 = (ctypes.c_float * 4)(1, 0, 0, 0)
    f12 = (ctypes.c_float * 12)(1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0)
    sh = (ctypes.c_float * 164)()
    p = [1] * 8                                                   # never dereferenced: every call below returns before a launch
    assert lib.ts_transform_gaussians(-1, 0, f12, f4, 0.0, None, None, *([None] * 8), None) == -1
    for k_rest in (-1, 1, 9, 16, 25):
        assert lib.ts_transform_gaussians(0, k_rest, f12, f4, 0.0, sh, None, *([None] * 8), None) == -1
    for k_rest in (0, 3, 8, 15, 24):
        assert lib.ts_transform_gaussians(0, k_rest, None, None, 0.0, None, None, *([None] * 8), None) == 0
    assert lib.ts_transform_gaussians(4, 0, None, f4, 0.0, None, None, *p, None) == -1
    assert lib.ts_transform_gaussians(4, 0, f12, None, 0.0, None, None, *p, None) == -1
    assert lib.ts_transform_gaussians(4, 3, f12, f4, 0.0, None, None, *p, None) == -1           # bands without matrices
    assert lib.ts_transform_gaussians(4, 0, f12, f4, 0.0, None, None, *([None] * 8), None) == -1
    for missing in (0, 1, 2, 4, 5, 6):
        args = list(p)
        args[missing] = None
        assert lib.ts_transform_gaussians(4, 0, f12, f4, 0.0, None, None, *args, None) == -1
    for missing in (3, 7):                                        # colors_rest is needed only where k_rest > 0
        args = list(p)
        args[missing] = None
        assert lib.ts_transform_gaussians(4, 3, f12, f4, 0.0, sh, None, *args, None) == -1
    bad12 = (ctypes.c_float * 12)(*f12)
    bad12[11] = float("nan")
    bad4 = (ctypes.c_float * 4)(float("inf"), 0, 0, 0)
    bad_sh = (ctypes.c_float * 164)()
    bad_sh[8] = float("nan")
    assert lib.ts_transform_gaussians(4, 0, bad12, f4, 0.0, None, None, *p, None) == -1
    assert lib.ts_transform_gaussians(4, 0, f12, bad4, 0.0, None, None, *p, None) == -1
    assert lib.ts_transform_gaussians(4, 0, f12, f4, float("inf"), None, None, *p, None) == -1
    assert lib.ts_transform_gaussians(4, 3, f12, f4, 0.0, bad_sh, None, *p, None) == -1
    assert lib.ts_box_mask(-1, f12, None, None, None) == -1 and lib.ts_box_mask(0, None, None, None, None) == 0
    assert lib.ts_box_mask(4, None, 1, 1, None) == -1 and lib.ts_box_mask(4, f12, None, 1, None) == -1
    assert lib.ts_box_mask(4, f12, 1, None, None) == -1 and lib.ts_box_mask(4, bad12, 1, 1, None) == -1
    assert lib.ts_abi_version() == 9


def test_module_refuses_cpu_tensors_and_held_models():
    model, _ = scene_args(10, 1, 16, 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        edit.transform_gaussians(model, TC.sim3())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        edit.box_mask(model, (0, 0, 0), (1, 1, 1))
    model.held_by = {"TrainStep"}
    with pytest.raises(RuntimeError, match="held by"):
        edit.transform_gaussians(model, TC.sim3())
    with pytest.raises(TypeError):
        edit.transform_gaussians(model, np.eye(4))
    for kw in (dict(half_extent=(1, 0, 1)), dict(half_extent=(1, np.nan, 1)), dict(center=(0, 0)), dict(rotation=np.eye(2))):
        with pytest.raises(ValueError):
            edit.box_mask(model, **{"center": (0, 0, 0), "half_extent": (1, 1, 1), **kw})


def _tool(name):
    spec = importlib.util.spec_from_file_location(f"tool_{name}_edit", str(ROOT / "tools" / f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_export_tool_flags(capsys):
    ex = _tool("export")
    base = ["in.ply", "out.ply", "--filetype", "PLY"]
    a = ex.parse(base)
    assert a.rotate is None and a.translate is None and a.scale is None and not a.orient_cameras and a.crop_box is None
    assert ex.scene_transform(a) is None
    a = ex.parse(base + ["--rotate", "0.3,-0.5,0.7,0.2", "--translate=-1,2,3.5", "--scale", "2.5", "--crop-box", "0,0,0,1,2,3"])
    assert a.rotate == [0.3, -0.5, 0.7, 0.2] and a.translate == [-1.0, 2.0, 3.5] and a.scale == 2.5
    assert a.crop_box == [0.0, 0.0, 0.0, 1.0, 2.0, 3.0]
    t = ex.scene_transform(a)
    assert np.abs(t.matrix() - Sim3.from_quat(TC.QUAT, (-1.0, 2.0, 3.5), 2.5).matrix()).max() < 1e-15
    only_scale = ex.scene_transform(ex.parse(base + ["--scale", "0.5"]))
    assert np.array_equal(only_scale.matrix(), np.diag([0.5, 0.5, 0.5, 1.0]))
    # --orient-cameras first, the manual similarity after it
    a = ex.parse(base + ["--orient-cameras", "--dataset-dir", "d", "--scale", "2"])
    cams = _ring((0.0, -1.0, 0.0), (1.0, 2.0, 3.0), 4.0)
    both = ex.scene_transform(a, cams)
    assert np.abs(both.matrix() - (Sim3.from_quat((1, 0, 0, 0), scale=2.0) @ edit.orient_from_cameras(cams)).matrix()).max() < 1e-15
    errors = [(["--orient-cameras"], "--orient-cameras needs --dataset-dir"),
              (["--dataset-dir", "d"], "--dataset-dir goes with --mesher tsdf or --semantic-dir"),
              (["--scale", "0"], "--scale must be positive"), (["--scale", "-2"], "--scale must be positive"),
              (["--scale", "nan"], "--scale must be positive"), (["--rotate", "0,0,0,0"], "not zero"),
              (["--rotate", "1,0,0"], "4 comma-separated"), (["--translate", "1,2,x"], "3 comma-separated"),
              (["--translate", "1,2,inf"], "finite"), (["--crop-box", "0,0,0,1,1"], "6 comma-separated"),
              (["--crop-box", "0,0,0,1,0,1"], "half extents > 0"), (["--crop-box", "0,0,0,1,-1,1"], "half extents > 0")]
    for extra, message in errors:
        with pytest.raises(SystemExit):
            ex.parse(base + extra)
        assert message in capsys.readouterr().err, extra
    # what was an error stays one, and what parsed still parses
    with pytest.raises(SystemExit):
        ex.parse(["in.ply", "out.obj", "--filetype", "OBJ", "--mesher", "tsdf"])
    assert "--dataset-dir goes with --mesher tsdf or --semantic-dir" in capsys.readouterr().err
    assert ex.parse(["in.ply", "out.obj", "--filetype", "OBJ", "--mesher", "tsdf", "--dataset-dir", "d", "--rotate", "1,0,0,1"]).mesher == "tsdf"


def test_train_tool_flag():
    tr = _tool("train")
    assert tr.parse_frame([]).normalize_scene is False and tr.parse_frame(["--normalize-scene", "--max-iter", "5"]).normalize_scene
    args = tr.parse(["--normalize-scene", "--max-iter", "5"])          # the main parser lets it through and does not hold it
    assert args.max_iter == 5 and not hasattr(args, "normalize_scene")
