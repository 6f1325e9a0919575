"""Per-vertex mesh attributes, host side: the PLY writer / reader with normals and colours, the normal transform under
scale_mat, the scripts' --vertex_colors flag, and the numpy fp32 mirror + synthetic scene tests/test_vertex_attrs_gpu.py uses."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- the small synthetic scene of the GPU tests (CPU tensors; the GPU tests move them) -------------------------------------
N_SAMPLES = [16, 8, 8, 8]
H, W, NV = 32, 64, 5
SEED = 0
BOUNDARY_BAND = 1e-5          # in units of c * 256, the value the quantisation truncates
MAX_EXCLUDED = 0.01


def make_model():
    """bench.model_conf's network, seeded; lin1..lin5 also read the sparse feature columns (the geometric initialisation zeroes
    them), so the surface and its gradient depend on the volumes."""
    from bench import model_conf
    from surf_amd.implicit_surface import ImplicitSurface
    torch.manual_seed(SEED)
    model = ImplicitSurface(model_conf(N_SAMPLES))
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        model.deviation_network.variance.fill_(0.45)
        for l in range(1, 6):
            wv = getattr(model.sdf_network, f"lin{l}").weight_v
            wv[:, -28:] += 0.03 * torch.randn(wv.shape[0], 28, generator=g)
    return model


def make_scene_cpu():
    """Ring cameras, procedural images, a random feature pyramid and the analytic sphere pyramid (__graft_entry__.smoke's scene
    with five views of 32 x 64): vertices near the poles of the r ~ 0.5 surface leave the narrow images, so the mesh holds
    every view count from 0 to NV - 1."""
    from surf_amd import synthetic
    intrs, c2ws, _ = synthetic.ring_cameras(NV, H, W)
    imgs = synthetic.procedural_images(NV, H, W, SEED, "cpu")
    feats = synthetic.feature_pyramid(NV, H, W, SEED, "cpu")
    vols, tabs, mvol = synthetic.sphere_pyramid(8, "cpu", bands=(float("inf"), 0.92, 0.3, 0.1))
    return dict(intrs=intrs, c2ws=c2ws, imgs=imgs, feats=feats, vols=vols[::-1], tabs=tabs[::-1], mvol=mvol)


def oracle_attributes(model, sc, pts):
    """The CPU oracle at fp32 points: (g (n,3) SDF gradient, c (n,3) blending colour, n_valid (n,) view counts)."""
    from oracle import surf_oracle as O
    sd = {"implicit_surface." + k: v.detach().cpu() for k, v in model.state_dict().items()}
    tabs = [t.long() for t in sc["tabs"]]
    phi, jphi = O.lookup_sparse_volume(pts, [v[:, :7] for v in sc["vols"]], tabs, with_jac=True)
    _, g, _ = O.sdf_mlp(O.sdf_weights(sd), pts, phi, jphi)
    rgb_feat, ray_diff, mvalid = O.lookup_feature(pts, sc["imgs"], sc["intrs"], sc["c2ws"], sc["feats"])
    c = O.blending(sd, rgb_feat, ray_diff, mvalid)
    return g, c, mvalid.long().sum(1)


def quantise(c):
    """validate's img_fine rule, then truncation: clip(c * 256, 0, 255) -> uint8 (numpy fp32)."""
    q = np.asarray(c, dtype=np.float32) * np.float32(256.0)
    return np.fmin(np.fmax(q, np.float32(0.0)), np.float32(255.0)).astype(np.uint8)


def near_boundary(c):
    """Rows with a channel whose c * 256 lies within BOUNDARY_BAND of a boundary between two levels, the integers 1 .. 255 (where
    truncation may flip on a last-bit difference; everything below 1 is level 0 and everything from 255 up is level 255, so 0 -
    the colour of a texel the reference's zero padding returns - and 256 are no boundaries)."""
    q = np.asarray(c, dtype=np.float64) * 256.0
    r = np.rint(q)
    return ((np.abs(q - r) < BOUNDARY_BAND) & (r >= 1) & (r <= 255)).any(axis=1)


def finish_mirror(grad, color, n_valid):
    """vertex_attrs.hip's finish stage in numpy fp32, operation by operation (the order of the file's header comment)."""
    f = np.float32
    g = np.asarray(grad, dtype=f)
    with np.errstate(all="ignore"):
        gx, gy, gz = g[:, 0], g[:, 1], g[:, 2]
        n = np.sqrt(((gx * gx).astype(f) + (gy * gy).astype(f)).astype(f) + (gz * gz).astype(f)).astype(f)
        ok = (n > f(0.0)) & (n <= np.finfo(f).max)
        safe = np.where(ok, n, f(1.0)).astype(f)
        normals = np.stack([np.where(ok, (gx / safe).astype(f), f(0.0)), np.where(ok, (gy / safe).astype(f), f(0.0)),
                            np.where(ok, (gz / safe).astype(f), f(0.0))], axis=1).astype(f)
        colors = quantise(color)
    colors = np.where((np.asarray(n_valid) == 0)[:, None], np.uint8(128), colors).astype(np.uint8)
    return normals, colors


# ---- tests -----------------------------------------------------------------------------------------------------------------


def _mesh(n=7):
    g = np.random.default_rng(5)
    v = g.standard_normal((n, 3))
    t = np.array([[0, 1, 2], [2, 3, 4], [4, 5, 6], [6, 0, 3]], dtype=np.int64)
    nrm = g.standard_normal((n, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    col = g.integers(0, 256, (n, 3)).astype(np.uint8)
    return v, t, nrm, col


def test_ply_round_trip_with_attributes(tmp_path):
    from surf_amd import mesh_io
    v, t, nrm, col = _mesh()
    for kw in (dict(normals=nrm, colors=col), dict(normals=nrm), dict(colors=col)):
        path = str(tmp_path / ("_".join(sorted(kw)) + ".ply"))
        mesh_io.write_ply(path, v, t, **kw)
        v2, t2, attrs = mesh_io.read_ply(path, attributes=True)
        assert np.array_equal(v2, v.astype(np.float32)) and np.array_equal(t2, t)
        assert sorted(attrs) == sorted(kw)
        for k in kw:
            assert attrs[k].dtype == kw[k].dtype and np.array_equal(attrs[k], kw[k])
        v3, t3 = mesh_io.read_ply(path)                                 # the two-value form skips the attributes
        assert np.array_equal(v3, v2) and np.array_equal(t3, t2)
        head = open(path, "rb").read().split(b"end_header\n")[0].decode()
        assert ("property float nx\nproperty float ny\nproperty float nz\n" in head) == ("normals" in kw)
        assert ("property uchar red\nproperty uchar green\nproperty uchar blue\n" in head) == ("colors" in kw)
        assert os.path.getsize(path) == len(head) + len("end_header\n") + len(v) * (12 + 12 * ("normals" in kw) + 3 * ("colors" in kw)) \
            + len(t) * 13
    # a bare file read with attributes=True: an empty dict
    bare = str(tmp_path / "bare.ply")
    mesh_io.write_ply(bare, v, t)
    assert mesh_io.read_ply(bare, attributes=True)[2] == {}
    with pytest.raises(ValueError):
        mesh_io.write_ply(bare, v, t, colors=col.astype(np.float32))
    with pytest.raises(ValueError):
        mesh_io.write_ply(bare, v, t, normals=nrm[:-1])


def test_ply_without_attributes_is_byte_identical(tmp_path):
    """The documented bare-geometry layout, assembled here from the header text and the raw arrays."""
    from surf_amd import mesh_io
    v, t, _, _ = _mesh()
    path = str(tmp_path / "bare.ply")
    mesh_io.write_ply(path, v, t)
    header = ("ply\nformat binary_little_endian 1.0\ncomment surf_amd mesh export\n"
              f"element vertex {len(v)}\nproperty float x\nproperty float y\nproperty float z\n"
              f"element face {len(t)}\nproperty list uchar int vertex_indices\nend_header\n")
    faces = b"".join(b"\x03" + row.astype("<i4").tobytes() for row in t)
    assert open(path, "rb").read() == header.encode("ascii") + v.astype("<f4").tobytes() + faces
    path2 = str(tmp_path / "bare2.ply")
    mesh_io.export_mesh(path2, v, t, None, normals=None, colors=None)
    assert open(path2, "rb").read() == open(path, "rb").read()


def _similarity(scale=187.5):
    a = np.linalg.qr(np.random.default_rng(2).standard_normal((3, 3)))[0]
    if np.linalg.det(a) < 0:
        a[:, 0] = -a[:, 0]
    m = np.eye(4)
    m[:3, :3] = scale * a
    m[:3, 3] = [30.0, -12.0, 640.0]
    return m


def test_normals_follow_scale_mat(tmp_path):
    from surf_amd import mesh_io
    v, t, nrm, col = _mesh()
    nrm[3] = 0.0                                                        # a zero row (no gradient) stays zero
    m = _similarity()
    ref = nrm.astype(np.float64) @ m[:3, :3].T
    ref = ref / np.maximum(np.linalg.norm(ref, axis=1, keepdims=True), 1e-300)
    ref[3] = 0.0
    out = mesh_io.transform_normals(nrm, m)
    assert out.dtype == np.float32 and np.array_equal(out[3], np.zeros(3, np.float32))
    assert np.abs(out.astype(np.float64) - ref).max() <= 2.0 ** -23     # float64 arithmetic, one rounding to fp32
    assert np.abs(np.linalg.norm(out[[0, 1, 2, 4, 5, 6]].astype(np.float64), axis=1) - 1.0).max() < 1e-6
    path = str(tmp_path / "world.ply")
    vw = mesh_io.export_mesh(path, v, t, torch.from_numpy(m), normals=nrm, colors=col)
    v2, t2, attrs = mesh_io.read_ply(path, attributes=True)
    assert np.array_equal(v2, mesh_io.transform_vertices(v, m).astype(np.float32)) and np.array_equal(vw, mesh_io.transform_vertices(v, m))
    assert np.array_equal(attrs["normals"], out) and np.array_equal(attrs["colors"], col)
    # geometry of the coloured file = geometry of the bare file
    bare = str(tmp_path / "world_bare.ply")
    mesh_io.export_mesh(bare, v, t, m)
    vb, tb = mesh_io.read_ply(bare)
    assert np.array_equal(vb, v2) and np.array_equal(tb, t2)
    # within the 1e-4 relative bound a slightly non-uniform scale passes, beyond it it does not
    ok = m.copy()
    ok[:3, 0] *= 1.0 + 2e-5
    mesh_io.transform_normals(nrm, ok)


def test_sheared_scale_mat_is_refused(tmp_path):
    from surf_amd import mesh_io
    v, t, nrm, col = _mesh()
    shear = _similarity()
    shear[:3, :3] = shear[:3, :3] @ np.array([[1.0, 0.01, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    with pytest.raises(ValueError):
        mesh_io.transform_normals(nrm, shear)
    with pytest.raises(ValueError):
        mesh_io.export_mesh(str(tmp_path / "s.ply"), v, t, shear, normals=nrm, colors=col)
    aniso = _similarity()
    aniso[:3, 1] *= 1.001
    with pytest.raises(ValueError):
        mesh_io.transform_normals(nrm, aniso)
    mesh_io.export_mesh(str(tmp_path / "s.ply"), v, t, shear)           # bare geometry: any matrix, as before
    mesh_io.export_mesh(str(tmp_path / "c.ply"), v, t, shear, colors=col)   # colours do not transform


def test_scripts_accept_vertex_colors():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import dtu_chamfer
    import finetune
    a = dtu_chamfer.parse_args(["--conf", "c", "--eval_dir", "e", "--vertex_colors"])
    assert a.vertex_colors is True
    assert dtu_chamfer.parse_args(["--conf", "c", "--eval_dir", "e"]).vertex_colors is False
    b = finetune.parse_args(["--conf", "c", "--resume", "r", "--vertex_colors"])
    assert b.vertex_colors is True
    assert finetune.parse_args(["--conf", "c", "--resume", "r"]).vertex_colors is False


def test_conf_key_defaults_off():
    from bench import model_conf
    from surf_amd.implicit_surface import ImplicitSurface
    conf = model_conf(N_SAMPLES)
    assert ImplicitSurface(conf).mesh_vertex_attributes is False
    conf["render"]["vertex_attributes"] = True
    assert ImplicitSurface(conf).mesh_vertex_attributes is True


def test_finish_mirror_rules():
    """The mirror itself on hand-made rows: unit normals, zero rows for zero / nan / inf / overflowing gradients, truncation,
    clipping, grey where no view sees the vertex."""
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    g = np.array([[3, 0, 4], [0, 0, 0], [nan, 1, 1], [inf, 0, 0], [3e38, 3e38, 0], [1e-30, 0, 0],
                  [2.0 ** -40, 0, 0]], dtype=np.float32)
    c = np.array([[0.5, -0.1, 1.5], [0.999, 0.00390624, 0.00390626], [0.1, 0.2, 0.3], [nan, 0, 1], [0, 0, 0], [1, 1, 1],
                  [1, 1, 1]], dtype=np.float32)
    k = np.array([1, 2, 0, 3, 1, 1, 4], dtype=np.uint8)
    n, q = finish_mirror(g, c, k)
    assert np.array_equal(n[0], np.array([0.6, 0.0, 0.8], np.float32))
    assert not n[1:6].any() and np.array_equal(n[6], np.array([1, 0, 0], np.float32))     # (1e-30)^2 underflows: |g| == 0
    assert q.tolist() == [[128, 0, 255], [255, 0, 1], [128, 128, 128], [0, 0, 255], [0, 0, 0], [255, 255, 255], [255, 255, 255]]


def test_oracle_colours_rarely_sit_on_a_quantisation_boundary():
    """For the GPU parity test's seed: of the oracle's own colours on the r = 0.5 sphere (where the geometric initialisation
    puts the surface) at most MAX_EXCLUDED of the points have a channel within BOUNDARY_BAND of a truncation boundary."""
    model, sc = make_model(), make_scene_cpu()
    g = torch.Generator().manual_seed(SEED)
    p = torch.randn(4000, 3, generator=g)
    p = (0.5 * p / p.norm(dim=1, keepdim=True)).float()
    _, c, nvalid = oracle_attributes(model, sc, p)
    seen = (nvalid > 0).numpy()
    assert 0.5 < seen.mean() < 1.0                                      # both seen and unseen points
    assert set(nvalid.tolist()) == set(range(NV))
    share = float(near_boundary(c.numpy()[seen]).mean())
    assert share <= MAX_EXCLUDED, share
