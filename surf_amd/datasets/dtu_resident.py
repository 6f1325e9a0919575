"""Device-resident DTU training set: `DTUDeviceTrainSet(dataset, device)` stands in front of a train-mode `DTUDataset` and returns,
for the same seeds, the dictionary `to_device(dataset[idx])` would - made on the device.

The host reader decodes five 1200 x 1600 PNGs, two mask PNGs, four PFMs and a PLY for every item and hands the runner 25.9 MB to
upload (img_hw 480 x 640, 5 views).  Here a file is read ONCE: what it holds after the nearest-neighbour pick is uploaded and kept
- texels and masks as uint8, depths as unscaled fp32 - and later items send the drawn indices, the cameras and the 2048 pseudo
points (about 52 KB in one buffer); `ops.train_views` / `ops.train_rays` (train_batch.hip) write the batch from the cache.

  host work per item (`plan`)    the reader's draws, in its order and from the same generators: numpy `src_idx`; torch `free_x`,
                                 `free_y`, the indices into the inside-mask pixel list (their `high` is the list's length, recorded
                                 when the mask was first read); numpy point-cloud indices (the cloud's size likewise).  Cameras go
                                 through the reader's `normalise_rig`, memoised per reference view: DTU's cameras are the same for
                                 every scan.  `pseudo_pts` stays on the host in fp64 - clouds are kept in host RAM after the first
                                 parse and the reader's own numpy lines transform the 2048 drawn points - and is uploaded (49 KB).
  cache entries (on a miss)      (scan, view, light): the image, uint8 (H, W, 3).  (scan, view): the mask uint8 0/1 (`> 10`), the
                                 int32 row-major flat indices of its pixels > 0.5, the ground-truth and the pseudo depth, fp32
                                 (H, W), unscaled.  The nearest-neighbour pick happens on the uint8 array (`mvs_io.resize_nearest`
                                 commutes with the conversion to fp32), and u8 / 256 is exact in fp32: `imgs` equals the reader's
                                 bit for bit.
  no eviction                    once `budget_bytes` is reached a new entry is uploaded for the item at hand and not kept
                                 (`stats.uncached`); the items are the same either way.

Everything returned is a fresh device tensor: nothing aliases the cache.  `rays_d` follows the fp32 operation order written out in
train_batch.hip, which differs from the host's matmuls by summation order only; every other entry is bit-equal to the reader's.
The set holds device memory: use it in the process that owns the device (`num_workers=0`; `get_loader(..., device=...)` does that).
"""
from types import SimpleNamespace

import numpy as np
import torch
from PIL import Image
from torch.utils.data import Dataset, get_worker_info

from . import mvs_io
from .dtu import DTUDataset, RawViews, normalise_rig

N_PSEUDO_PTS = 2048           # datasets/dtu.py:440


def _read_u8(path, hw, channels):
    """The file as uint8, nearest-neighbour picked to hw: what `read_image` returns, before its conversion to fp32."""
    a = np.array(Image.open(path))
    want = 3 if channels else 2
    if a.dtype != np.uint8 or a.ndim != want or (channels and a.shape[2] != channels):
        raise ValueError(f"{path}: the device-resident set holds 8-bit {'RGB images' if channels else 'grey masks'}, got "
                         f"{a.dtype} {a.shape}")
    return np.ascontiguousarray(mvs_io.resize_nearest(a, hw))


def _inside_list(mask01):
    """Row-major flat indices of the pixels with mask > 0.5: `torch.nonzero(mask > 0.5)` as y * W + x."""
    return np.flatnonzero(mask01.reshape(-1)).astype(np.int32)


class DTUDeviceTrainSet(Dataset):
    def __init__(self, dataset, device, budget_bytes=64 << 30):
        if not isinstance(dataset, DTUDataset) or dataset.mode != "train":
            raise TypeError("DTUDeviceTrainSet: expected a DTUDataset in train mode")
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError(f"DTUDeviceTrainSet: expected a GPU device, got {device} (the host reader is the CPU path)")
        self.dataset, self.device, self.budget_bytes = dataset, device, int(budget_bytes)
        self.stats = SimpleNamespace(hits=0, misses=0, resident_bytes=0, uploaded_bytes=0, uncached=0)
        self._images, self._views = {}, {}        # the device cache
        self._inside_count = {}                   # (scan, view) -> length of the inside list, recorded when the mask was read
        self._pending = {}                        # the one mask read by plan() ahead of its upload: key -> (mask01, inside)
        self._clouds, self._cams, self._rigs = {}, {}, {}
        # fp32 array * np.float64 scalar: float64 under NumPy 2's promotion (then cast), fp32 with the scalar demoted under NumPy 1
        self._demote_scale = (np.ones(1, np.float32) * np.float64(1)).dtype == np.float32

    def __len__(self):
        return len(self.dataset)

    def __getattr__(self, name):                  # conf attributes (img_hw, n_rays, metas, ...) read through to the host reader
        if name == "dataset":
            raise AttributeError(name)
        return getattr(self.dataset, name)

    # ---- the host half ------------------------------------------------------------------------------------------------
    def _camera(self, vid):
        if vid not in self._cams:
            self._cams[vid] = self.dataset.read_cam(self.dataset.files.camera(vid))
        return self._cams[vid]

    def _rig(self, view_ids):
        """normalise_rig of the item's cameras + what the ray kernel takes of the reference camera; one per reference view."""
        key = tuple(view_ids)
        if key not in self._rigs:
            cams = [self._camera(v) for v in view_ids]
            raw = RawViews([], [c[0] for c in cams], [c[1] for c in cams], [c[2] for c in cams], [])
            rig = normalise_rig(self.dataset.img_hw, raw, self.dataset.factor)
            kinv = torch.inverse(rig.intrs[0])[:3, :3].contiguous().numpy().reshape(-1)             # host fp32, as pixel_rays
            c2w = rig.c2ws[0][:3, :4].contiguous().numpy().reshape(-1)
            scale = float(np.float32(rig.scale_factor)) if self._demote_scale else float(rig.scale_factor)
            self._rigs[key] = SimpleNamespace(rig=rig, w2c_ref=raw.w2cs[0], kinv=kinv, c2w=c2w, scale=scale,
                                              scale_mat=rig.ref_c2w_raw @ rig.scale_mat)
        return self._rigs[key]

    def _host_mask(self, scan, vid):
        key = (scan, vid)
        if key not in self._pending:
            mask01 = (_read_u8(self.dataset.files.mask(scan, vid), self.dataset.img_hw, 0) > 10).astype(np.uint8)
            inside = _inside_list(mask01)
            self._inside_count[key] = int(inside.shape[0])
            self._pending = {key: (mask01, inside)}
        return self._pending[key]

    def _cloud(self, scan):
        if scan not in self._clouds:
            self._clouds[scan] = mvs_io.read_ply_points(self.dataset.files.pseudo_points(scan))
        return self._clouds[scan]

    def plan(self, idx, pixels=False):
        """The host half of item idx, no GPU needed: the reader's five draws in its order, the cameras, `pseudo_pts`.  The first
        plan of a (scan, reference view) reads its mask file (for the inside count) and of a scan its point cloud.  pixels=True
        adds the host's `pixels_x` / `pixels_y` (reads the reference mask again unless it is still at hand)."""
        ds = self.dataset
        scan, light, ref_view = ds.metas[idx]
        view_ids = [ref_view] + list(ds.pairs[ref_view])[:ds.num_src_view]
        src_idx = np.random.randint(1, len(view_ids))                                # draw 1 (numpy)
        cam = self._rig(view_ids)
        H, W = ds.img_hw
        if ds.n_rays <= 0:
            raise AssertionError("No sampling rays!")
        if (scan, ref_view) not in self._inside_count:
            self._host_mask(scan, ref_view)
        n_free = ds.n_rays // 4
        free_x = torch.randint(low=0, high=W, size=[n_free])                         # draws 2 - 4 (torch), as choose_pixels
        free_y = torch.randint(low=0, high=H, size=[n_free])
        pick = torch.randint(low=0, high=self._inside_count[(scan, ref_view)], size=[ds.n_rays - n_free])
        cloud = self._cloud(scan)
        cloud = cloud[np.random.randint(low=0, high=cloud.shape[0], size=[N_PSEUDO_PTS])]          # draw 5 (numpy)
        cloud_h = np.concatenate([cloud, np.ones_like(cloud[..., :1])], axis=1)
        in_ref = np.matmul(cam.w2c_ref, cloud_h[..., None])[:, :3, 0]
        rig = cam.rig
        out = SimpleNamespace(scan=scan, light=light, view_ids=view_ids, src_idx=src_idx, free_x=free_x, free_y=free_y, pick=pick,
                              cam=cam, intrs=rig.intrs, c2ws=rig.c2ws, near_fars=rig.near_fars, scale_mat=torch.from_numpy(cam.scale_mat),
                              pseudo_pts=torch.from_numpy((in_ref - rig.scale_mat[:3, 3][None]) / rig.scale_mat[0, 0]))
        if pixels:
            flat = torch.from_numpy(self._host_mask(scan, ref_view)[1].astype(np.int64))[pick]
            out.pixels_x = torch.cat([(flat % W).float(), free_x.float()])
            out.pixels_y = torch.cat([torch.div(flat, W, rounding_mode="floor").float(), free_y.float()])
        return out

    # ---- the device cache ---------------------------------------------------------------------------------------------
    def _upload(self, array):
        array = np.ascontiguousarray(array)
        self.stats.uploaded_bytes += array.nbytes
        return torch.from_numpy(array).to(self.device)

    def _keep(self, cache, key, entry, nbytes):
        if self.stats.resident_bytes + nbytes <= self.budget_bytes:
            cache[key] = entry
            self.stats.resident_bytes += nbytes
        else:
            self.stats.uncached += 1
        return entry

    def _image(self, scan, vid, light):
        key = (scan, vid, light)
        if key in self._images:
            self.stats.hits += 1
            return self._images[key]
        self.stats.misses += 1
        img = _read_u8(self.dataset.files.image(scan, vid, light), self.dataset.img_hw, 3)
        return self._keep(self._images, key, self._upload(img), img.nbytes)

    def _view(self, scan, vid):
        key = (scan, vid)
        if key in self._views:
            self.stats.hits += 1
            return self._views[key]
        self.stats.misses += 1
        ds = self.dataset
        mask01, inside = self._host_mask(scan, vid)
        self._pending = {}
        depth, pseudo = (np.ascontiguousarray(ds.read_depth(f(scan, vid)), dtype=np.float32) for f in (ds.files.depth, ds.files.pseudo_depth))
        entry = SimpleNamespace(mask=self._upload(mask01), inside=self._upload(inside), depth=self._upload(depth), pseudo=self._upload(pseudo))
        return self._keep(self._views, key, entry, mask01.nbytes + inside.nbytes + depth.nbytes + pseudo.nbytes)

    def warm(self, indices):
        """Fill the cache with everything the items `indices` can ask for (every source view can be the supervised one).  Draws
        nothing from the random generators."""
        self._check_process()
        ds = self.dataset
        for idx in indices:
            scan, light, ref_view = ds.metas[idx]
            for vid in [ref_view] + list(ds.pairs[ref_view])[:ds.num_src_view]:
                self._image(scan, vid, light)
                self._view(scan, vid)

    @staticmethod
    def _check_process():
        if get_worker_info() is not None:
            raise RuntimeError("DTUDeviceTrainSet holds device memory and must run in the process that owns the device: build the "
                               "DataLoader with num_workers=0 (get_loader(..., device=...) does)")

    def _upload_packed(self, parts):
        """Host arrays -> ONE upload; returns {name: its device tensor}, views of disjoint 16-byte aligned pieces of that buffer."""
        at, total = {}, 0
        for name, a in parts.items():
            total = (total + 15) & ~15
            at[name] = total
            total += a.nbytes
        buf = np.zeros(total, np.uint8)
        for name, a in parts.items():
            buf[at[name]:at[name] + a.nbytes] = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
        dev = self._upload(buf)
        return {name: dev[at[name]:at[name] + a.nbytes].view(torch.from_numpy(a[:0]).dtype).reshape(a.shape) for name, a in parts.items()}

    def __getitem__(self, idx):
        from .. import ops
        self._check_process()
        p = self.plan(idx)
        ref, src = p.view_ids[0], p.view_ids[p.src_idx]
        images = [self._image(p.scan, v, p.light) for v in p.view_ids]
        e_ref, e_src = self._view(p.scan, ref), self._view(p.scan, src)
        small = self._upload_packed({"pseudo_pts": p.pseudo_pts.numpy(), "scale_mat": p.scale_mat.numpy(),
                                     "view_ids": np.array(p.view_ids).astype(np.int64), "intrs": p.intrs.numpy(), "c2ws": p.c2ws.numpy(),
                                     "near_fars": p.near_fars.numpy(), "pick": p.pick.numpy().astype(np.int32),
                                     "free_x": p.free_x.numpy().astype(np.int32), "free_y": p.free_y.numpy().astype(np.int32)})
        scale = p.cam.scale
        imgs, masks, depths, pseudos = ops.train_views(images, [e_ref.mask, e_src.mask], [e_ref.depth, e_src.depth],
                                                       [e_ref.pseudo, e_src.pseudo], scale)
        rays = ops.train_rays(small["pick"], small["free_x"], small["free_y"], e_ref.inside, p.cam.kinv, p.cam.c2w, images[0], e_ref.mask,
                              e_ref.depth, e_ref.pseudo, scale)
        near_fars = small["near_fars"]
        return {"imgs": imgs, "intrs": small["intrs"], "c2ws": small["c2ws"], "scale_mat": small["scale_mat"], "view_ids": small["view_ids"],
                "pixels_x": rays["pixels_x"], "pixels_y": rays["pixels_y"], "rays_o": rays["rays_o"], "rays_d": rays["rays_d"],
                "near": near_fars[0, 0].reshape(1, 1), "far": near_fars[0, 1].reshape(1, 1), "near_fars": near_fars,
                "pseudo_pts": small["pseudo_pts"], "color": rays["color"], "depth": rays["depth"], "pseudo_depth": rays["pseudo_depth"],
                "mask": rays["mask"], "mask_ref": masks[0], "depth_ref": depths[0], "pseudo_depth_ref": pseudos[0],
                "pseudo_depth_src": pseudos[1], "src_idx": p.src_idx, "mask_src": masks[1], "depth_src": depths[1]}
