"""Per-scene fine-tuning reader (datasets/dtu_finetune.py:75-345 `DTUDatasetFinetune`): ONE scene, the reference view and its two
best source views, read once; `get_all_images()` feeds `SuRF.init_volumes`, `get_random_rays(vid)` is the batch of a step and
`get_rays_at(vid)` the validation lattice.  Contractual, and pinned to the reference's reader (tests/test_dtu_finetune.py against
tests/golden/finetune_items.npz): conf keys, file names, the dictionaries' keys / dtypes / shapes, and the order of the three
draws of a step - `randint(W, [n_rays])`, `randint(H, [n_rays])`, `randint(n_pts, [2048])` on torch's CPU default generator - so
that a seeded run picks the reference's pixels and pseudo points.  The file formats and the camera algebra are those of
surf_amd.datasets.dtu / mvs_io.

Two ways to make a batch:

  host    (as read)                 the reference's: indexing and ray algebra on the host; the caller uploads the dictionary -
                                    `imgs` included, 3 x 3 x H x W fp32 = 69 MB a step at 1200 x 1600.
  device  (`dataset.to("cuda")`)    images, masks, pseudo depths, pseudo points, cameras and the per-view inverse(K) (computed on
                                    the host in fp32, `intrs[vid].inverse()` as the reference does, so the same 9 numbers) are
                                    uploaded ONCE.  A step then uploads one packed int32 buffer - the drawn x, y and point
                                    indices, 2 n_rays + 2048 values, 12 KB at 512 rays - and `ops.finetune_rays` /
                                    `ops.finetune_gather_pts` (finetune_rays.hip) make the batch there.  Every entry is a device
                                    tensor; `rays_d` follows the fp32 operation order written out in finetune_rays.hip, which
                                    differs from the host's matmuls by summation order only.

`imgs` of the device path: the three orderings `images[[vid] + others]` are built on the device at their first use and CACHED,
(3, 3, H, W) contiguous each - 207 MB at 1200 x 1600 for all three, on a 288 GB device - rather than gathered every step: a step
then touches no image-sized memory at all before the model reads it.  The cached tensors are returned as they are: read-only for
the caller (an in-place write is caught at the next call through the tensors' version counters).  The validation lattice is
built once with the reference's own host calls (`torch.linspace` on the CPU, `meshgrid`) and uploaded: `linspace(0, 1599, 400)`
passes through exact integers, and a device linspace landing one ulp below one of them would truncate to the neighbouring pixel.

`pseudo_pts`: mvs_io.read_ply_points returns float64 columns, so the host path's rows are float64 (as surf_amd.datasets.dtu's
and as the fixture's); the device path holds them as fp32, what the kernels read (`ImplicitSurface.pseudo_sdf` casts to it).
"""
import numpy as np
import torch
from torch.utils.data import Dataset

from . import mvs_io
from .dtu import DTUFiles, RawViews, _f32, normalise_rig, pixel_rays, scale_intrinsics

N_PSEUDO_PTS = 2048           # datasets/dtu_finetune.py:279


class DTUFinetuneFiles(DTUFiles):
    """The fine-tuning reader's own places under data_dir (datasets/dtu_finetune.py:107-121): light 3 of Rectified_raw,
    PseudoMVSScore/dtu_exp/{scan}/filtered_avg_depth/{vid:08d}.pfm, PseudoMVSDepth/mvsnet{scan number:03d}_l3.ply."""

    def image(self, scan, vid, light=3):
        return self.path("Rectified_raw", scan, "rect_{:0>3}_{}_r5000.png".format(vid + 1, light))

    def pseudo_depth(self, scan, vid):
        return self.path("PseudoMVSScore", "dtu_exp", scan, "filtered_avg_depth", "{:0>8}.pfm".format(vid))

    def pseudo_points(self, scan):
        return self.path("PseudoMVSDepth", "mvsnet{:0>3}_l3.ply".format(int(scan[4:])))


def _ordered(vid, n):
    """[vid] + the other views in ascending order (dtu_finetune.py:282)."""
    return [vid] + list(range(n))[:vid] + list(range(n))[vid + 1:]


class DTUDatasetFinetune(Dataset):
    RAW_HW = (1200, 1600)

    def __init__(self, confs, mode):
        super().__init__()
        self.mode = mode
        self.data_dir = confs["data_dir"]
        self.interval_scale = confs.get_float("interval_scale")
        self.num_interval = confs.get_int("num_interval")
        self.img_hw = [int(v) for v in confs["img_hw"]]
        self.n_rays = confs.get_int("n_rays")
        self.factor = confs.get_float("factor")
        self.num_views = 3
        self.scene = confs.get_string("scene")
        self.ref_view = confs.get_int("ref_view")
        self.val_res_level = confs.get_int("val_res_level", default=1)
        self.files = DTUFinetuneFiles(self.data_dir)
        self.pairs = mvs_io.read_pair_file(self.files.path("Cameras", "pair.txt"))
        self.all_views = [self.ref_view] + list(self.pairs[self.ref_view])[:self.num_views - 1]

        raw = RawViews([], [], [], [], [])
        depths = []
        for vid in self.all_views:
            K, w2c, near_far = mvs_io.read_cam_file(self.files.camera(vid), self.interval_scale, self.num_interval)
            raw.intrs.append(scale_intrinsics(K, self.img_hw, self.RAW_HW))
            raw.w2cs.append(w2c)
            raw.near_fars.append(near_far)
            raw.imgs.append(mvs_io.read_image(self.files.image(self.scene, vid), self.img_hw) / 256.0)
            raw.masks.append((mvs_io.read_image(self.files.mask(self.scene, vid), self.img_hw) > 10).astype(np.float32))
            depths.append(mvs_io.resize_nearest(mvs_io.read_pfm(self.files.pseudo_depth(self.scene, vid))[0], self.img_hw))
        rig = normalise_rig(self.img_hw, raw, self.factor)
        self.intrs, self.c2ws, self.near_fars = rig.intrs, rig.c2ws, rig.near_fars
        self.scale_factor = rig.scale_factor
        self.w2c_ref = raw.w2cs[0]
        self.w2c_ref_inv = _f32(rig.ref_c2w_raw)
        self.images = _f32(np.stack(raw.imgs))                                     # (3, H, W, 3)
        self.masks = _f32(np.stack(raw.masks))                                     # (3, H, W)
        self.pseudo_depths = _f32(np.stack(depths)) * self.scale_factor           # (3, H, W), normalised frame
        # pseudo surface points: into the reference view's frame, then into the unit sphere - with the scale_mat of the
        # normalisation itself (dtu_finetune.py:128), BEFORE it is composed with the reference pose (dtu_finetune.py:130)
        scale_mat = _f32(rig.scale_mat)
        cloud = mvs_io.read_ply_points(self.files.pseudo_points(self.scene))
        cloud_h = np.concatenate([cloud, np.ones_like(cloud[..., :1])], axis=1)
        in_ref = torch.from_numpy(np.matmul(self.w2c_ref, cloud_h[..., None])[:, :3, 0])
        self.pseudo_pts = (in_ref - scale_mat[:3, 3][None]) / scale_mat[0, 0]
        self.scale_mat = self.w2c_ref_inv @ scale_mat
        self.device = torch.device("cpu")
        self._dev = None
        self.uploaded_bytes = 0          # host -> device bytes this reader has sent (tests bound the per-step share)

    # ---- the reference's host path ---------------------------------------------------------------------------------
    def get_all_images(self):
        if self._dev is not None:
            d = self._dev
            return {"imgs": self._view_order(0)[2], "c2ws": d["c2ws"], "intrs": d["intrs"], "near": d["near"][0], "far": d["far"][0],
                    "near_fars": d["near_fars"]}
        near, far = self.near_fars[0].reshape(1, 2).split(split_size=1, dim=1)
        return {"imgs": self.images.permute(0, 3, 1, 2), "c2ws": self.c2ws, "intrs": self.intrs, "near": near, "far": far,
                "near_fars": self.near_fars}

    def draw(self):
        """The three draws of a step, in the reference's order (dtu_finetune.py:265-266, 279)."""
        px = torch.randint(low=0, high=self.img_hw[1], size=[self.n_rays])
        py = torch.randint(low=0, high=self.img_hw[0], size=[self.n_rays])
        idx = torch.randint(low=0, high=self.pseudo_pts.shape[0], size=[N_PSEUDO_PTS])
        return px, py, idx

    def _host_rays(self, vid, px, py):
        at = (py.long(), px.long())
        rays_o, rays_d = pixel_rays(px, py, self.intrs[vid], self.c2ws[vid])
        near, far = self.near_fars[vid].reshape(1, 2).split(split_size=1, dim=1)
        view_ids = _ordered(vid, self.num_views)
        return {"rays_o": rays_o, "rays_d": rays_d, "near": near, "far": far, "color": self.images[vid][at],
                "intrs": self.intrs[view_ids], "c2ws": self.c2ws[view_ids], "view_ids": view_ids,
                "imgs": self.images[view_ids].permute(0, 3, 1, 2)}, at

    def get_random_rays(self, vid):
        vid = int(vid.item()) if torch.is_tensor(vid) else int(vid)
        px, py, idx = self.draw()
        if self._dev is not None:
            return self._device_random_rays(vid, px, py, idx)
        out, at = self._host_rays(vid, px, py)
        out.update(pseudo_pts=self.pseudo_pts[idx], pseudo_depth=self.pseudo_depths[vid][at])
        return out

    def lattice(self):
        """(x, y) of the validation lattice, row-major, by the reference's own host calls (dtu_finetune.py:304-307)."""
        H, W = self.img_hw
        tx = torch.linspace(0, W - 1, W // self.val_res_level)
        ty = torch.linspace(0, H - 1, H // self.val_res_level)
        gy, gx = torch.meshgrid(ty, tx, indexing="ij")
        return gx.reshape(-1), gy.reshape(-1)

    def get_rays_at(self, vid):
        vid = int(vid.item()) if torch.is_tensor(vid) else int(vid)
        if self._dev is not None:
            return self._device_rays_at(vid)
        px, py = self.lattice()
        out, _ = self._host_rays(vid, px, py)
        H, W = self.img_hw
        out.update(scale_mat=self.scale_mat, scene=self.scene, masks=self.masks[out["view_ids"]],
                   bound_min=torch.tensor([-1, -1, -1], dtype=torch.float32), bound_max=torch.tensor([1, 1, 1], dtype=torch.float32),
                   hw=torch.Tensor([H // self.val_res_level, W // self.val_res_level]).int())
        return out

    # ---- the device path -------------------------------------------------------------------------------------------
    def _upload(self, t, dev):
        t = t.contiguous()
        self.uploaded_bytes += t.numel() * t.element_size()
        return t.to(dev)

    def to(self, device):
        """Upload the scene once (a CPU device: back to the host path).  Needs the kernel library."""
        device = torch.device(device)
        if device.type == "cpu":
            self.device, self._dev = device, None
            return self
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if self._dev is not None and self.device == device:      # already there: the upload and the caches stay
            return self
        from .. import ops  # noqa: F401  (a missing library is an error here, not at the first step)
        up = lambda t: self._upload(t, device)                                                   # noqa: E731
        kinv = torch.stack([self.intrs[v].inverse()[:3, :3].reshape(-1) for v in range(self.num_views)])       # host fp32
        near_fars = up(self.near_fars)
        self._dev = {"images": up(self.images), "depths": up(self.pseudo_depths), "masks": up(self.masks),
                     "pts": up(self.pseudo_pts.float()), "intrs": up(self.intrs), "c2ws": up(self.c2ws), "near_fars": near_fars,
                     "kinv": up(kinv), "c2w_rows": up(self.c2ws[:, :3, :4].reshape(self.num_views, 12)),
                     "near": [near_fars[v, 0].reshape(1, 1) for v in range(self.num_views)],
                     "far": [near_fars[v, 1].reshape(1, 1) for v in range(self.num_views)],
                     "scale_mat": up(self.scale_mat), "bound_min": up(torch.tensor([-1, -1, -1], dtype=torch.float32)),
                     "bound_max": up(torch.tensor([1, 1, 1], dtype=torch.float32)),
                     "hw": up(torch.Tensor([self.img_hw[0] // self.val_res_level, self.img_hw[1] // self.val_res_level]).int()),
                     "order": {}, "lattice": None}
        self.device = device
        return self

    def cuda(self, device=None):
        return self.to("cuda" if device is None else torch.device("cuda", device))

    def _view_order(self, vid):
        """(intrs, c2ws, imgs (3, 3, H, W), masks) in the order [vid] + others: built on the device once per vid and cached."""
        d = self._dev
        if vid not in d["order"]:
            ids = _ordered(vid, self.num_views)
            pick = lambda t: torch.stack([t[i] for i in ids])                                    # noqa: E731  (device copies)
            entry = (pick(d["intrs"]), pick(d["c2ws"]), pick(d["images"]).permute(0, 3, 1, 2).contiguous(), pick(d["masks"]))
            d["order"][vid] = (entry, [t._version for t in entry])
        entry, versions = d["order"][vid]
        if [t._version for t in entry] != versions:              # handed out as they are, every step: an in-place write by a
            raise RuntimeError("DTUDatasetFinetune: a cached device tensor (imgs / intrs / c2ws / masks) was modified in place; "
                               "the reader returns them read-only")       # caller would corrupt every later batch
        return entry

    def _device_random_rays(self, vid, px, py, idx):
        from .. import ops
        d, n = self._dev, self.n_rays
        packed = self._upload(torch.cat([px, py, idx]).to(torch.int32), self.device)            # the step's only upload
        rays_o, rays_d, color, pseudo_depth = ops.finetune_rays(packed[:n], packed[n:2 * n], d["kinv"][vid], d["c2w_rows"][vid],
                                                                d["images"][vid], d["depths"][vid])
        intrs, c2ws, imgs, _ = self._view_order(vid)
        return {"rays_o": rays_o, "rays_d": rays_d, "near": d["near"][vid], "far": d["far"][vid], "color": color, "intrs": intrs,
                "c2ws": c2ws, "view_ids": _ordered(vid, self.num_views), "imgs": imgs,
                "pseudo_pts": ops.finetune_gather_pts(d["pts"], packed[2 * n:]), "pseudo_depth": pseudo_depth}

    def _device_rays_at(self, vid):
        from .. import ops
        d = self._dev
        if d["lattice"] is None:
            d["lattice"] = tuple(self._upload(t, self.device) for t in self.lattice())
        px, py = d["lattice"]
        rays_o, rays_d, color, _ = ops.finetune_rays(px, py, d["kinv"][vid], d["c2w_rows"][vid], d["images"][vid], None)
        intrs, c2ws, imgs, masks = self._view_order(vid)
        return {"rays_o": rays_o, "rays_d": rays_d, "near": d["near"][vid], "far": d["far"][vid], "color": color, "intrs": intrs,
                "c2ws": c2ws, "view_ids": _ordered(vid, self.num_views), "scale_mat": d["scale_mat"], "scene": self.scene,
                "imgs": imgs, "masks": masks, "bound_min": d["bound_min"], "bound_max": d["bound_max"], "hw": d["hw"]}
