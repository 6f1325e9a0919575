"""The host path of the DTU protocol's mesh cleaner (surf_amd.evaluation.clean_dtu) against the reference's recorded results
(tests/golden/clean_dtu.npz, made by tests/golden/make_golden_clean_dtu.py from evaluation/clean_mesh.py) and against
constructed cases whose answer follows from the definition.

The reference projects with np.matmul, which has no defined summation order; this module evaluates one float64 operation per
operator.  The two can differ by an ulp of X / Z, which changes a rounded pixel only at a tie, so the golden comparison leaves
out the vertices whose float64 X / Z or Y / Z lies within BAND = 1e-6 px of a half-integer in some view (an ulp near 1600 px
is 2e-13 px; 1e-6 px is generous and still expected to exclude about 1e-5 of random vertices, i.e. none of 8000).  At most 0.1 %
may be excluded, and when none is, full equality is demanded."""
import os
import sys

import numpy as np
import pytest

from surf_amd import mesh_io
from surf_amd.evaluation import clean_dtu as D
from surf_amd.evaluation import clean_mesh as CM
from tests.golden import dtu_test_scene as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAND, CAP = 1e-6, 1e-3
IDENTITY = np.eye(4, dtype=np.float32)


# ---- shared with tests/test_clean_dtu_gpu.py -----------------------------------------------------------------------------------

def near_tie(vertices, P_list, band=BAND):
    near = np.zeros(len(vertices), dtype=bool)
    for P in P_list:
        qx, qy, _ = D._project(vertices, P)
        with np.errstate(all="ignore"):
            for q in (qx, qy):
                near |= np.abs(np.abs(q - np.floor(q)) - 0.5) < band
    return near


_GOLDEN = {}


def golden():
    """The recorded reference results plus the scene's masks and their host dilation (made once, never written to)."""
    if not _GOLDEN:
        z = np.load(os.path.join(ROOT, "tests", "golden", "clean_dtu.npz"))
        _GOLDEN.update({k: z[k] for k in z.files})
        _GOLDEN["masks"] = S.masks()
        _GOLDEN["dilated"] = [D.dilate_ellipse(m, 11) for m in _GOLDEN["masks"]]
        _GOLDEN["near"] = near_tie(_GOLDEN["vertices"], _GOLDEN["P"])
        for a in _GOLDEN.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return _GOLDEN


def check_against_golden(count, clean_vertices, clean_faces):
    """count (V,) and the first stage's mesh (minimal_vis 1) against the reference, under the band and its cap."""
    g = golden()
    near = g["near"]
    print(f"near a rounding tie: {int(near.sum())} of {len(near)} vertices")
    assert near.mean() <= CAP
    for mv in (0, 1, 2):
        ours, ref = count > mv, g[f"inside_minvis{mv}"]
        print(f"minimal_vis {mv}: {int(ours.sum())} kept here, {int(ref.sum())} in the reference, "
              f"{int((ours != ref)[~near].sum())} differ off the band")
        assert np.array_equal(ours[~near], ref[~near])
    if not near.any():
        assert np.array_equal(clean_vertices, g["clean_vertices"]) and np.array_equal(clean_faces, g["clean_faces"])
    else:                                   # the faces none of whose vertices is on the band, by their (exact) coordinates
        ok = ~near[g["faces"]].any(axis=1)
        ref_keep = g["inside_minvis1"][g["faces"]].all(axis=1)
        ours_keep = (count > 1)[g["faces"]].all(axis=1)
        assert np.array_equal(ours_keep[ok], ref_keep[ok])


def constructed_cases():
    """Points for P = [I | 0] (qx = x / z, qy = y / z) on 6 x 8 masks, with the number of views (of the two: an even-column
    mask and an all-zero mask) the definition gives each.  Returns (points, P_list, masks, expected count)."""
    h, w = 6, 8
    even = np.zeros((h, w), dtype=np.uint8)
    even[:, 0::2] = 255                     # a tie k + 0.5 rounds to the even neighbour: always a set column of this mask
    zero = np.zeros((h, w), dtype=np.uint8)
    pts, want = [], []

    def add(x, y, z, n):
        pts.append((x * z, y * z, z))
        want.append(n)
    for k in range(0, w - 1):
        add(k + 0.5, 2.0, 1.0, 1)           # half to even: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, ...
        add(k + 0.5, 2.5, 1.0, 1)           # rows too: 2.5 -> 2
    add(1.0, 2.0, 1.0, 0)                   # an odd column: unset in both masks
    add(1.4999999, 2.0, 1.0, 0)
    add(1.5000001, 2.0, 1.0, 1)
    # the ring and its asymmetric range: u = rint(x) + 1 in {-1, 0, W, W + 1}
    add(-2.0, 2.0, 1.0, 0)                  # u = -1: out of range
    add(-1.0, 2.0, 1.0, 2)                  # u = 0: the ring, whatever the masks hold
    add(w - 1.0, 2.0, 1.0, 0)               # u = W: the last column (odd: unset)
    add(w - 2.0, 2.0, 1.0, 1)               # u = W - 1: the last even column
    add(float(w), 2.0, 1.0, 0)              # u = W + 1: on the ring but not in range
    add(2.0, -2.0, 1.0, 0)
    add(2.0, -1.0, 1.0, 2)                  # v = 0: the ring
    add(3.0, -1.0, 1.0, 2)
    add(2.0, h - 1.0, 1.0, 1)               # v = H: the last row
    add(2.0, float(h), 1.0, 0)              # v = H + 1
    add(-1.0, -1.0, 1.0, 2)                 # the ring's corner
    add(-1.0, float(h), 1.0, 0)
    add(-0.5, 2.0, 1.0, 1)                  # rint(-0.5) = -0: u = 1, column 0 (set in `even` only), not the ring
    add(-1.5, 2.0, 1.0, 0)                  # rint(-1.5) = -2: u = -1
    # Z < 0 is counted like Z > 0 (the reference does not test the sign)
    add(2.0, 2.0, -2.0, 1)
    add(-1.0, 3.0, -0.5, 2)
    add(1.0, 2.0, -3.0, 0)
    # Z == 0 and overflow are not counted
    pts.append((2.0, 2.0, 0.0)); want.append(0)
    pts.append((0.0, 0.0, 0.0)); want.append(0)
    pts.append((1e300, 2.0, 1e-300)); want.append(0)
    pts.append((2.0, -1e300, 1e-300)); want.append(0)
    pts.append((float(2 ** 31), 2.0, 1.0)); want.append(0)
    pts.append((-float(2 ** 40), -1.0, 1.0)); want.append(0)
    pts.append((float(2 ** 62), float(2 ** 62), 1.0)); want.append(0)
    pts.append((float("nan"), 2.0, 1.0)); want.append(0)
    pts.append((float("inf"), 2.0, 1.0)); want.append(0)
    return (np.array(pts, dtype=np.float64), [IDENTITY, IDENTITY], [even, zero], np.array(want, dtype=np.int32))


def grid_mesh(n=30, half=60.0, z=0.0):
    """A connected plane of 2 (n-1)^2 faces in world millimetres, facing the ring cameras."""
    ax = np.linspace(-half, half, n)
    xx, yy = np.meshgrid(ax, ax, indexing="ij")
    v = np.stack([xx.ravel(), yy.ravel(), np.full(n * n, z)], axis=1)
    i = (np.arange(n - 1)[:, None] * n + np.arange(n - 1)[None, :]).ravel()
    f = np.concatenate([np.stack([i, i + n, i + 1], axis=1), np.stack([i + 1, i + n, i + n + 1], axis=1)])
    return v, f.astype(np.int64)


# ---- tests ---------------------------------------------------------------------------------------------------------------------

def test_points_in_masks_and_vertex_removal_equal_the_reference():
    g = golden()
    count = D.points_in_masks(g["vertices"], g["P"], g["dilated"], dilate=None)
    assert count.dtype == np.int32 and np.array_equal(count, D.points_in_masks(g["vertices"], g["P"], g["masks"], dilate=11))
    v1, f1 = D.clean_faces_by_mask(g["vertices"], g["faces"], count, 1)
    check_against_golden(count, v1, f1)
    # unreferenced vertices stay: the first stage's vertex list is exactly the kept vertices
    assert len(v1) == int((count > 1).sum()) > len(np.unique(f1))


def test_ellipse_footprint_table():
    assert D.ellipse_footprint(1).tolist() == [[True]]
    assert D.ellipse_footprint(3).astype(int).tolist() == [[0, 1, 0], [1, 1, 1], [0, 1, 0]]
    fp = D.ellipse_footprint(11)
    assert fp.shape == (11, 11) and fp.sum(axis=1).tolist() == [1, 7, 9, 11, 11, 11, 11, 11, 9, 7, 1]
    assert np.array_equal(fp, fp[::-1]) and np.array_equal(fp, fp[:, ::-1]) and fp[0, 5] and fp[1, 2] and not fp[1, 1]
    with pytest.raises(ValueError):
        D.ellipse_footprint(10)
    with pytest.raises(ValueError):
        D.dilate_ellipse(np.zeros((4, 4), np.uint8), 10)


def brute_dilate(m, k):
    fp = D.ellipse_footprint(k)
    r = k // 2
    h, w = m.shape
    out = np.zeros_like(m)
    for y in range(h):
        for x in range(w):
            best = 0
            for i in range(k):
                for j in range(k):
                    yy, xx = y + i - r, x + j - r
                    if fp[i, j] and 0 <= yy < h and 0 <= xx < w:
                        best = max(best, int(m[yy, xx]))
            out[y, x] = best
    return out


def dilation_masks(h, w, seed=0):
    """Grey uint8 masks with sparse values, touching every border and every corner; plus all-zero and all-set."""
    g = np.random.default_rng(seed)
    a = np.where(g.random((h, w)) < 0.03, g.integers(1, 256, (h, w)), 0).astype(np.uint8)
    a[0, 0], a[0, w - 1], a[h - 1, 0], a[h - 1, w - 1] = 200, 90, 255, 129
    a[0, w // 2], a[h - 1, w // 3], a[h // 2, 0], a[h // 3, w - 1] = 17, 128, 250, 3
    return [a, np.zeros((h, w), np.uint8), np.full((h, w), 255, np.uint8)]


@pytest.mark.parametrize("k", [1, 3, 11])
def test_dilation_equals_a_brute_force_maximum(k):
    for h, w in ((17, 23), (9, 5)):                           # the second is smaller than the 11 x 11 footprint
        for m in dilation_masks(h, w):
            assert np.array_equal(D.dilate_ellipse(m, k), brute_dilate(m, k))


def test_constructed_rounding_ring_sign_and_overflow_cases():
    pts, P_list, masks, want = constructed_cases()
    got = D.points_in_masks(pts, P_list, masks, dilate=None)
    assert got.tolist() == want.tolist(), [(p, int(a), int(b)) for p, a, b in zip(pts.tolist(), got, want) if a != b]
    # an all-set mask: the ring's asymmetry is all that is left (u = W + 1 / v = H + 1 are out, u = 0 / v = 0 are in)
    full = np.full((6, 8), 255, np.uint8)
    edge = np.array([[-1.0, 2, 1], [8.0, 2, 1], [7.0, 2, 1], [2.0, -1, 1], [2.0, 6, 1], [2.0, 5, 1]])
    assert D.points_in_masks(edge, [IDENTITY], [full], dilate=None).tolist() == [1, 0, 1, 1, 0, 1]
    # the threshold is > 128
    grey = np.full((6, 8), 128, np.uint8)
    grey[2, 3] = 129
    assert D.points_in_masks(np.array([[3.0, 2, 1], [4.0, 2, 1]]), [IDENTITY], [grey], dilate=None).tolist() == [1, 0]


def test_clean_faces_by_mask_keeps_order_and_unreferenced_vertices():
    v = np.arange(18, dtype=np.float64).reshape(6, 3)
    f = np.array([[0, 1, 2], [2, 3, 5], [5, 3, 2], [1, 2, 4]])
    count = np.array([2, 2, 3, 2, 1, 2], dtype=np.int32)      # vertex 4 goes, and face 3 with it
    v1, f1 = D.clean_faces_by_mask(v, f, count, 1)
    assert np.array_equal(v1, v[[0, 1, 2, 3, 5]]) and f1.tolist() == [[0, 1, 2], [2, 3, 4], [4, 3, 2]]
    v0, f0 = D.clean_faces_by_mask(v, f, count, 2)            # only vertex 2 is kept: no face, one unreferenced vertex
    assert np.array_equal(v0, v[[2]]) and f0.shape == (0, 3)
    ve, fe = D.clean_faces_by_mask(v[:0], f[:0], count[:0], 1)
    assert ve.shape == (0, 3) and fe.shape == (0, 3)


def test_projection_matrix_is_float32_k4_times_e(tmp_path):
    cams = S.write_tree(str(tmp_path), scans=())
    P = D.projection_matrix(str(tmp_path / "cameras" / f"{S.VIEW_IDS[1]:08d}_cam.txt"))
    assert P.dtype == np.float32 and P.shape == (4, 4) and np.array_equal(P[3], [0, 0, 0, 1])
    K4 = np.eye(4)
    K4[:3, :3] = S.K
    assert np.allclose(P, K4 @ cams[1], rtol=1e-5, atol=1e-2)
    assert np.array_equal(P, golden()["P"][1])


def test_read_ply_mesh_round_trip(tmp_path):
    g = np.random.default_rng(0)
    v = g.standard_normal((50, 3)).astype(np.float32)
    f = g.integers(0, 50, (80, 3))
    mesh_io.write_ply(str(tmp_path / "a.ply"), v, f)
    rv, rf = mesh_io.read_ply_mesh(str(tmp_path / "a.ply"))
    assert rv.dtype == np.float64 and rf.dtype == np.int64 and np.array_equal(rv, v.astype(np.float64)) and np.array_equal(rf, f)
    mesh_io.write_ply(str(tmp_path / "b.ply"), v, f, normals=v, colors=g.integers(0, 256, (50, 3)).astype(np.uint8))
    rv, rf = mesh_io.read_ply_mesh(str(tmp_path / "b.ply"))
    assert np.array_equal(rv, v.astype(np.float64)) and np.array_equal(rf, f)
    with open(tmp_path / "c.ply", "w") as fh:
        fh.write("ply\nformat ascii 1.0\nelement vertex 4\nproperty double x\nproperty double y\nproperty double z\n"
                 "element face 2\nproperty list uchar int vertex_indices\nend_header\n"
                 "0 0 0\n1 0 0.5\n0 1 0\n1 1 1e-3\n3 0 1 2\n3 2 1 3\n")
    rv, rf = mesh_io.read_ply_mesh(str(tmp_path / "c.ply"))
    assert rv.tolist() == [[0, 0, 0], [1, 0, 0.5], [0, 1, 0], [1, 1, 1e-3]] and rf.tolist() == [[0, 1, 2], [2, 1, 3]]
    mesh_io.write_ply(str(tmp_path / "e.ply"), v[:0], f[:0])
    rv, rf = mesh_io.read_ply_mesh(str(tmp_path / "e.ply"))
    assert rv.shape == (0, 3) and rf.shape == (0, 3)


def test_cli_file_names_and_view_sets(tmp_path, monkeypatch):
    """Two scans, both view sets: set 1's views carry the scene's masks, set 0's views empty ones.  The z-buffer first hit needs
    a GPU; this test is about files and view selection, so it replaces that one call by "every face is seen" (the whole cleaner
    runs in tests/test_clean_dtu_gpu.py)."""
    root, out = tmp_path / "DTU_TEST", tmp_path / "meshes"
    S.write_tree(str(root), scans=(24, 37))
    set0 = D.VIEW_SETS[0][:3]
    S.write_tree(str(root), scans=(24, 37), view_ids=set0, mask_list=[np.zeros((S.H, S.W), np.uint8)] * 3)
    assert D.VIEW_SETS[1][:3] == S.VIEW_IDS and not set(set0) & set(S.VIEW_IDS)
    v, f = grid_mesh()
    os.makedirs(out)
    mesh_io.write_ply(str(out / "surf_scan24_epoch0.ply"), v, f)
    mesh_io.write_ply(str(out / "x_scan37_epoch0.ply"), v + np.array([10.0, 0, 0]), f)
    monkeypatch.setattr(CM, "visible_faces", lambda vertices, faces, *a, **k: np.ones(len(faces), dtype=bool))
    D.main(["--root_dir", str(root), "--out_dir", str(out), "--scans", "24", "37", "--backend", "host"])
    assert sorted(os.listdir(out / "final")) == ["clean_024.ply", "clean_037.ply", "scan24.ply", "scan37.ply"]
    _, P_list, masks = D.read_scan_views(str(root), 24, 1, 3)
    v32 = v.astype(np.float32).astype(np.float64)
    want_v, want_f = D.clean_faces_by_mask(v32, f, D.points_in_masks(v32, P_list, masks, 11), 1)
    cv, cf = mesh_io.read_ply_mesh(str(out / "final" / "clean_024.ply"))
    assert 0 < len(want_f) < len(f) and np.array_equal(cv, want_v) and np.array_equal(cf, want_f)
    fv, ff = mesh_io.read_ply_mesh(str(out / "final" / "scan24.ply"))
    keep = CM.face_components(want_f, 500)
    assert keep.sum() >= 500 and len(ff) == int(keep.sum()) and len(fv) == len(np.unique(want_f[keep]))
    assert len(mesh_io.read_ply_mesh(str(out / "final" / "scan37.ply"))[1]) > 0
    # the other view set reads the other masks (empty: only the ring of ones could count, and the plane is inside the images)
    D.main(["--root_dir", str(root), "--out_dir", str(out), "--scans", "24", "--set", "0", "--n_view", "3"])
    cv, cf = mesh_io.read_ply_mesh(str(out / "final" / "clean_024.ply"))
    assert len(cv) == 0 and len(cf) == 0 and len(mesh_io.read_ply_mesh(str(out / "final" / "scan24.ply"))[1]) == 0
    with pytest.raises(SystemExit):
        D.main(["--root_dir", str(root), "--out_dir", str(out), "--scans", "55"])


def test_chamfer_script_defaults_to_the_runner_cleaner():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import dtu_chamfer
    a = dtu_chamfer.parse_args(["--conf", "c", "--eval_dir", "e"])
    assert a.clean_protocol == "runner" and a.clean_set == 1 and a.dtu_test_dir is None and not a.clean_mesh
    b = dtu_chamfer.parse_args(["--conf", "c", "--eval_dir", "e", "--clean_mesh", "--clean_protocol", "dtu_test", "--dtu_test_dir", "d",
                                "--clean_set", "0", "--clean_backend", "device"])
    assert (b.clean_protocol, b.dtu_test_dir, b.clean_set, b.clean_backend) == ("dtu_test", "d", 0, "device")
