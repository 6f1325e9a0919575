"""Torch-facing wrappers of the C-ABI kernels (device memory and streams are PyTorch's; the math is HIP).

Every function checks dtype / device / contiguity, allocates outputs with torch and launches on the
current stream.  Nothing here computes on the CPU except the one-off weight re-layouts (host code of
the library) and 4x4 camera inversions.
"""
import ctypes
import os
import time

import numpy as np
import torch

from . import _lib

BLEND_KEYS = ["s"] + [f"{m}.{i}.{p}" for m, idxs in (("ray_dir_fc", (0, 2)), ("base_fc", (0, 2)), ("vis_fc", (0, 2)),
                                                      ("vis_fc2", (0, 2)), ("rgb_fc", (0, 2, 4)))
                      for i in idxs for p in ("weight", "bias")]


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# bench.py: a list that receives (name, start event, end event, algorithmic units) of the instrumented backward launches
# (HIP events on the launch stream); None = no timing
kernel_events = None


class _timed:
    """with _timed("costvol_bwd", units): ... - brackets the launches inside with a HIP event pair when a bench asked for it."""

    def __init__(self, name, units=0):
        self.name, self.units = name, units

    def __enter__(self):
        if kernel_events is not None:
            self.a, self.b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            self.a.record()
        return self

    def __exit__(self, *exc):
        if kernel_events is not None and exc[0] is None:
            self.b.record()
            kernel_events.append((self.name, self.a, self.b, self.units))
        return False


class SideStream:
    """The backward sweep of a training step on several HIP streams.  Its kernels work on the step's 65 k samples or wait on row
    gathers / an LDS hash: latency bound, a fraction of the chip's wave slots each - so branches that do not depend on one
    another run side by side (users, each an A/B switch; profiles/r06_side_streams.txt):
      unet    the sparse U-Nets' kernel gradients (leaves of the sweep) beside their input-gradient chain          lane 0
      render  the colour branch (lane 0) and the smooth (H.1) branch (lane 1) beside the SDF value / gradient branch
      match   the matching chain (matching-field backward -> densify backward, fine -> coarse) ahead of the U-Net / cost-volume
              chain it feeds, one event per stage                                                                 lane 2
      costvol the stages' cost-volume backward (a leaf: only the parent-feature scatter feeds the next stage)           lane 2 (reused)
      loss    the 2 n photometric terms of the loss, both directions (autograd._PhotometricMulti; lanes 4..7; measured: a loss of
              1.5 ms - the launches are bound by the memory system, not by latency; off by default)
      fpn     the FPN's weight gradients (measured: a loss - those launches fill the chip; off by default)
      fwd     the forward's smooth / random-point branches and the frozen matching FPN (measured: no gain; off by default)
    `with side.fork(lane): launch(...)` orders the lane after everything issued so far on the current stream; `run(fn)` does that
    and marks the results for the current stream; `keep()` holds operands until `join()` (the caching allocator reuses a block
    for the CURRENT stream as soon as its last reference dies); `join()` makes the current stream wait for every open lane -
    before the results are read.  Never inside a lane: a synchronising host read (it starves the other streams).
    SURF_SIDE_STREAM=0: in-order launches."""

    def __init__(self):
        # "0" none, "1" the users that measured a gain (profiles/r06_side_streams.txt), "all", or a comma list of users
        env = os.environ.get("SURF_SIDE_STREAM", "1")
        self.enabled = env != "0"
        self.users = {"0": set(), "1": {"unet", "render", "match", "costvol"}, "all": None}.get(env, set(env.split(",")))
        self.priority = int(os.environ.get("SURF_SIDE_PRIORITY", "0"))      # of the lanes' streams (0 = as the current stream's)
        self._streams = {}
        self._keep = {}          # (device, lane) -> tensors held until that lane is joined
        self._open = set()

    def active(self, user=None):
        # never while a bench is bracketing launches with event pairs (per-kernel times want in-order launches)
        return (self.enabled and kernel_events is None and torch.cuda.is_available()
                and (self.users is None or user is None or user in self.users))

    def fork(self, lane=0):
        cur = torch.cuda.current_stream()
        key = (cur.device.index, lane)
        st = self._streams.get(key)
        if st is None:
            st = self._streams[key] = torch.cuda.Stream(device=cur.device, priority=self.priority)
        st.wait_stream(cur)
        self._open.add(key)
        return torch.cuda.stream(st)

    def lane_stream(self, lane, device=None):
        """The stream object of `lane` on `device` (default: the current one), created on first use, NOT ordered after anything:
        for graph nodes that LIVE on a lane - autograd runs a node's backward on the stream its forward ran on and orders the
        gradients that cross streams itself."""
        idx = torch.cuda.current_device() if device is None else torch.device(device).index
        key = (idx, lane)
        st = self._streams.get(key)
        if st is None:
            st = self._streams[key] = torch.cuda.Stream(device=torch.device("cuda", idx), priority=self.priority)
        return st

    def on_lane(self, lane):
        """True when the current stream is the stream of `lane`."""
        st = self._streams.get((torch.cuda.current_device(), lane))
        return st is not None and torch.cuda.current_stream() == st

    def run(self, fn, lane=0, keep=()):
        """fn() on side stream `lane`; its result tensors (a tensor, or a list / tuple / dict of them, nested) are allocated in
        that stream's pool and will be read - and freed - on the current one: marked with record_stream."""
        main = torch.cuda.current_stream()
        with self.fork(lane):
            out = fn()

        def claim(o):
            if torch.is_tensor(o):
                if o.is_cuda:
                    o.record_stream(main)
            elif isinstance(o, dict):
                for v in o.values():
                    claim(v)
            elif isinstance(o, (list, tuple)):
                for v in o:
                    claim(v)

        claim(out)
        self.keep(*keep, lane=lane)
        return out

    @staticmethod
    def mark():
        """An event on the CURRENT stream (inside `with fork(lane)`: that lane) for `wait_for` on another stream."""
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream())
        return ev

    @staticmethod
    def wait_for(event):
        torch.cuda.current_stream().wait_event(event)

    def keep(self, *tensors, lane=0):
        """Hold `tensors` (operands a lane reads, allocated on another stream) until that lane is joined."""
        if torch.cuda.is_available():
            key = (torch.cuda.current_device(), lane)
            self._keep.setdefault(key, []).extend(t for t in tensors if t is not None)

    def join(self, lanes=None):
        """The current stream waits for the open lanes of its device (all of them, or `lanes`)."""
        if not self._open:
            self._keep.clear()
            return
        cur = torch.cuda.current_stream()
        for key in sorted(self._open):
            if key[0] == cur.device.index and (lanes is None or key[1] in lanes):
                cur.wait_stream(self._streams[key])
                self._open.discard(key)
                self._keep.pop(key, None)


side = SideStream()
# The runtime multiplexes HIP streams onto a handful of hardware queues (4 by default): which streams share one decides how much really
# overlaps, and a fifth stream (or RCCL's own) reshuffles the assignment.  The cost-volume backward therefore REUSES the matching
# chain's lane (which ran ahead and is idle by then) instead of opening another stream: main + three lanes in all.  Measured on the
# default line's step (ms, group present / absent, two runs each): own lane 67.3 65.1 / 65.3 64.3, smooth lane 67.2 64.5 / 66.1 66.0,
# matching lane 65.5 63.5 / 64.5 64.5; under DistributedDataParallel 69.9 70.9 | 70.6 66.2 | 65.2 66.3.
# graph nodes that live on the matching lane (the depth tap, the loss's photometric node): autograd runs their backward there (A/B: 0 =
# the tap on the main stream forks the lane itself, the photometric terms run on the main stream)
lane_nodes = os.environ.get("SURF_LANE_NODES", "1") != "0"
COSTVOL_LANE = int(os.environ.get("SURF_COSTVOL_LANE", "2"))
SMOOTH_LANE = int(os.environ.get("SURF_SMOOTH_LANE", "1"))       # the render backward's smooth branch (A/B: 0 = behind the colour branch)


class _ZeroPool:
    """Small zero-initialised buffers carved out of one pre-zeroed block per device: a training step asks for ~100 of them
    (the 27 x C_in x C_out weight-gradient accumulators of the sparse U-Net, 1.2 MB a stage) and each torch.zeros is a ~5 us
    fill launch on a stream that is never idle.  A slice is handed out ONCE (never recycled: it lives as long as its views do),
    the block is replaced when it runs out."""
    BLOCK = 4 << 20          # floats (16 MB)
    LIMIT = 1 << 18          # larger requests fill for themselves

    def __init__(self):
        self._blocks = {}

    def take(self, shape, device):
        n = 1
        for d in shape:
            n *= int(d)
        if n > self.LIMIT or n == 0:
            return torch.zeros(shape, dtype=torch.float32, device=device)
        key = (device.type, device.index)
        blk = self._blocks.get(key)
        step = (n + 63) & ~63   # 256-byte slices
        if blk is None or blk[1] + step > self.BLOCK:
            blk = [torch.zeros(self.BLOCK, dtype=torch.float32, device=device), 0]
            self._blocks[key] = blk
        out = blk[0][blk[1]:blk[1] + n].view(shape)
        blk[1] += step
        return out


_zero_pool = _ZeroPool()


def small_zeros(shape, device):
    """fp32 zeros(shape) on `device`, from the pool above when small."""
    return _zero_pool.take(tuple(shape), torch.device(device))


def _p(t):
    t = getattr(t, "tensor", t)            # PackedBlend
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _chk(t, dtype, name, dev=True):
    if not torch.is_tensor(t) or t.dtype != dtype or not t.is_contiguous():
        raise TypeError(f"{name}: expected a contiguous {dtype} tensor")
    if dev and not t.is_cuda:
        raise TypeError(f"{name}: expected a GPU tensor (the SuRF hot path has no CPU fallback)")
    return t


def _host_f32(t):
    return np.ascontiguousarray(t.detach().to("cpu", torch.float32).numpy())


def _ptr_array(tensors):
    arr = (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
    return arr


def _np_ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _host_ptr_array(arrays):
    """The `const float* const*` of host arrays (the seven weight matrices / biases of an SDF network)."""
    return (ctypes.c_void_p * len(arrays))(*[a.ctypes.data for a in arrays])


# ------------------------------------------------------------------------------------------------
# layout helpers
# ------------------------------------------------------------------------------------------------


def pack_texel4(x):
    """(n, C<=4, H, W) fp32 NCHW -> (n, H, W, 4) texel4 (surf_pack_texel4)."""
    _chk(x, torch.float32, "x")
    n, C, H, W = x.shape
    out = torch.empty(n, H, W, 4, dtype=torch.float32, device=x.device)
    _lib.lib().surf_pack_texel4(_p(x), n, C, H, W, _p(out), _stream())
    return out


class SparseVolumes:
    """Per-stage sparse feature rows + dense int32 index tables, ordered fine -> coarse (surf.py:159)."""

    def __init__(self, feats, tables):
        self.vols, self.tables, self.dims = [], [], []
        for f, t in zip(feats, tables):
            if f.shape[1] != 8 or f.shape[0] == 0:   # the kernels read row 0 (with weight 0) for empty corners
                f8 = torch.zeros(max(f.shape[0], 1), 8, dtype=torch.float32, device=f.device)
                f8[:, :f.shape[1]] = f
                f = f8
            if t.dtype != torch.int32:
                t = t.to(torch.int32)
            self.vols.append(_chk(f.contiguous(), torch.float32, "sparse volume"))
            self.tables.append(_chk(t.contiguous(), torch.int32, "index table"))
            assert t.dim() == 3 and t.shape[0] == t.shape[1] == t.shape[2], "index tables must be cubic"
            self.dims.append(int(t.shape[0]))
        self.n = len(self.vols)
        self._vp = _ptr_array(self.vols)
        self._tp = _ptr_array(self.tables)
        self._dp = (ctypes.c_int * self.n)(*self.dims)


def sdf_effective_weights(sd, prefix="implicit_surface.sdf_network."):
    """weight_norm(dim=0) re-parameterisation (sdf_network.py:88-89): W = g * v / ||v||_row."""
    out = []
    for l in range(7):
        if f"{prefix}lin{l}.weight_v" in sd:
            v = sd[f"{prefix}lin{l}.weight_v"].detach().to("cpu", torch.float32)
            g = sd[f"{prefix}lin{l}.weight_g"].detach().to("cpu", torch.float32)
            W = v * (g / torch.linalg.norm(v, dim=1, keepdim=True))
        else:
            W = sd[f"{prefix}lin{l}.weight"].detach().to("cpu", torch.float32)
        out.append((W.contiguous(), sd[f"{prefix}lin{l}.bias"].detach().to("cpu", torch.float32).contiguous()))
    return out


def sdf_pack_weights_host(layers):
    """[(W_l, b_l)] effective matrices -> packed numpy buffer (surf_sdf_pack_weights, host code)."""
    shapes = [(128, 27), (128, 156), (101, 156), (128, 156), (128, 156), (128, 156)]
    for l, (W, b) in enumerate(layers):
        if l < 6 and tuple(W.shape) != shapes[l]:
            raise NotImplementedError(
                f"lin{l}.weight has shape {tuple(W.shape)}; the HIP SDF kernel implements the shipped architecture "
                "(d_hidden 128, n_layers 6, skip_in [3], multires 4, feat_channels 28)")
    if layers[6][0].shape[1] != 156:
        raise NotImplementedError("lin6 must take 156 inputs")
    Ws = [_host_f32(W) for W, _ in layers]
    bs = [_host_f32(b) for _, b in layers]
    L = _lib.lib()
    out = np.zeros(L.surf_sdf_packed_floats(), dtype=np.float32)
    wp, bp = _host_ptr_array(Ws), _host_ptr_array(bs)
    L.surf_sdf_pack_weights(wp, bp, _np_ptr(out))
    return out


SDF_PRECISIONS = ("f32", "bf16x3", "f16x2")
# the blend kernels of the library (render.blend_precision): "f32" = blend.hip (fp32 MFMA, register-resident weights
# stream, round 1); the others = blend_split.hip (weights resident in LDS, two wavefronts per SIMD): "f32lds" fp32 MFMA,
# "bf16x3" exact three-way bf16 split, "f16x2" two fp16 pieces
BLEND_PRECISIONS = ("f32", "f32lds", "bf16x3", "f16x2")
BLEND_DEFAULT = "bf16x3"
_BLEND_ID = {"bf16x3": 1, "f16x2": 2, "f32lds": 3}   # SURF_BLEND_BF16X3 / SURF_BLEND_F16X2 / SURF_BLEND_F32
_SPLIT_ABI = {"bf16x3": "bf16", "f16x2": "f16"}   # precision -> infix of the C-ABI entry points


def sdf_pack_weights_split_host(layers, precision):
    """[(W_l, b_l)] effective matrices -> byte stream of split 16-bit weights (surf_sdf_pack_weights_{bf16,f16})."""
    sdf_pack_weights_host(layers)  # shape validation only
    infix = _SPLIT_ABI[precision]
    Ws = [_host_f32(W) for W, _ in layers]
    bs = [_host_f32(b) for _, b in layers]
    L = _lib.lib()
    out = np.zeros(getattr(L, f"surf_sdf_{infix}_packed_bytes")(), dtype=np.uint8)
    wp, bp = _host_ptr_array(Ws), _host_ptr_array(bs)
    getattr(L, f"surf_sdf_pack_weights_{infix}")(wp, bp, _np_ptr(out))
    return out


def sdf_pack_weights_bf16_host(layers):
    return sdf_pack_weights_split_host(layers, "bf16x3")


def sdf_pack_weights_split(sd, device, prefix="implicit_surface.sdf_network.", precision="bf16x3"):
    return torch.from_numpy(sdf_pack_weights_split_host(sdf_effective_weights(sd, prefix), precision)).to(device)


def sdf_pack_weights_bf16(sd, device, prefix="implicit_surface.sdf_network."):
    return sdf_pack_weights_split(sd, device, prefix, "bf16x3")


def sdf_packed_precision(packed):
    """Which SDF kernel a packed weight tensor belongs to (fp32 tensors: the fp32 kernel; byte streams: by size)."""
    if packed.dtype == torch.float32:
        return "f32"
    if packed.dtype == torch.uint8:
        for precision, infix in _SPLIT_ABI.items():
            if packed.numel() == getattr(_lib.lib(), f"surf_sdf_{infix}_packed_bytes")():
                return precision
    raise ValueError("packed SDF weights: not an output of surf_sdf_pack_weights / _bf16 / _f16")


def sdf_pack_weights(sd, device, prefix="implicit_surface.sdf_network."):
    return torch.from_numpy(sdf_pack_weights_host(sdf_effective_weights(sd, prefix))).to(device)


def blend_raw_weights(sd, prefix="implicit_surface.color_network."):
    return np.concatenate([_host_f32(sd[prefix + k]).reshape(-1) for k in BLEND_KEYS])


def blend_pack_weights_host(raw):
    L = _lib.lib()
    if raw.size != L.surf_blend_raw_floats():
        raise NotImplementedError("colour network shape differs from the shipped BlendingNetwork(d_feature=16)")
    out = np.zeros(L.surf_blend_packed_floats(), dtype=np.float32)
    L.surf_blend_pack_weights(_np_ptr(np.ascontiguousarray(raw, dtype=np.float32)), _np_ptr(out))
    return out


def blend_pack_weights_split_host(raw, precision):
    """LDS image of the split blend kernels (surf_blend_pack_weights_split): 16-bit weight pieces + bias / dot rows."""
    L = _lib.lib()
    if raw.size != L.surf_blend_raw_floats():
        raise NotImplementedError("colour network shape differs from the shipped BlendingNetwork(d_feature=16)")
    pid = _BLEND_ID[precision]
    out = np.zeros(L.surf_blend_split_packed_bytes(pid), dtype=np.uint8)
    L.surf_blend_pack_weights_split(_np_ptr(np.ascontiguousarray(raw, dtype=np.float32)), _np_ptr(out), pid)
    return out


class PackedBlend:
    """The LDS image of a split blend kernel together with the precision it was laid out for.  The f16x2 and f32lds images have
    the SAME size, so the layout cannot be recovered from the bytes: it travels with them explicitly (an attribute on the
    tensor, as in round 2, is lost by clone() / to() / a state-dict round trip and the f32lds image then ran through the f16x2
    kernel without any error)."""
    __slots__ = ("tensor", "precision")

    def __init__(self, tensor, precision):
        if precision not in _BLEND_ID:
            raise ValueError(f"blend precision must be one of {sorted(_BLEND_ID)}")
        if tensor.dtype != torch.uint8 or tensor.numel() != _lib.lib().surf_blend_split_packed_bytes(_BLEND_ID[precision]):
            raise ValueError(f"not a {precision} image of surf_blend_pack_weights_split")
        self.tensor, self.precision = tensor, precision

    def to(self, device):
        return PackedBlend(self.tensor.to(device), self.precision)

    @property
    def device(self):
        return self.tensor.device


def blend_pack_weights(sd, device, prefix="implicit_surface.color_network.", precision="f32"):
    """Packed BlendingNetwork weights for the blend kernel of `precision` (fp32 tensor: blend.hip; PackedBlend: blend_split.hip)."""
    raw = blend_raw_weights(sd, prefix)
    if precision == "f32":
        return torch.from_numpy(blend_pack_weights_host(raw)).to(device)
    return PackedBlend(torch.from_numpy(blend_pack_weights_split_host(raw, precision)).to(device), precision)


def blend_packed_precision(packed):
    """Which blend kernel a packed weight object belongs to.  Raw byte tensors are accepted only where the size identifies
    the layout; an ambiguous size raises instead of guessing."""
    if isinstance(packed, PackedBlend):
        return packed.precision
    if packed.dtype == torch.float32:
        return "f32"
    if packed.dtype == torch.uint8:
        hits = [precision for precision, pid in _BLEND_ID.items() if packed.numel() == _lib.lib().surf_blend_split_packed_bytes(pid)]
        if len(hits) == 1:
            return hits[0]
        if len(hits) > 1:
            raise ValueError(f"a {packed.numel()}-byte blend image fits the layouts {hits}: pass the PackedBlend that "
                             "blend_pack_weights returned (it carries the precision)")
    raise ValueError("packed blend weights: not an output of surf_blend_pack_weights / surf_blend_pack_weights_split")


# ------------------------------------------------------------------------------------------------
# kernels
# ------------------------------------------------------------------------------------------------


_linspace_cache = {}


_nf_cache = {}


def _near_fars_host(near_fars):
    """The (nv, 2) near / far planes as a host array (the kernels take them by value).  A device tensor costs a synchronising
    copy: paid once per tensor (keyed by storage address + version), not once per stage and direction - and never from inside
    a side-stream section of the backward sweep, where a host stall starves the other streams (ops.SideStream)."""
    if not near_fars.is_cuda:
        return np.ascontiguousarray(near_fars.detach().to(torch.float32).numpy())
    key = (near_fars.data_ptr(), near_fars._version, tuple(near_fars.shape), near_fars.dtype)
    hit = _nf_cache.get(key)
    if hit is None:
        if len(_nf_cache) >= 16:
            _nf_cache.clear()
        # the tensor itself is kept: a live tensor's address cannot be handed to another one
        hit = _nf_cache[key] = (near_fars, np.ascontiguousarray(near_fars.detach().to("cpu", torch.float32).numpy()))
    return hit[1]


def _linspace_dev(lo, hi, n, dev):
    """torch.linspace computed on the CPU - like the reference, whose sample fractions are CPU linspaces moved to the device
    (implicit_surface.py:271, matching_field.py:31) - and kept on the device: one host-to-device copy per (lo, hi, n), not one
    per call (a pageable copy is a synchronising operation)."""
    key = (float(lo), float(hi), int(n), str(dev))
    t = _linspace_cache.get(key)
    if t is None:
        t = torch.linspace(float(lo), float(hi), int(n), dtype=torch.float32).to(dev)
        _linspace_cache[key] = t
    return t


def ray_setup(rays_o, rays_d, near, far, mvol, volumes, n_samples, sample_ranges, n_depth, want_z=False, jitter=None):
    """implicit_surface.py:268-311 + :72-86.  Returns dict(mid_z, dists, pts, vmask[, z_vals]).
    jitter: None (render.perturb = 0) or (R, n_stage) float32 on the device = the `torch.rand([R, 1]) - 0.5` draws of
    render.perturb > 0, one column per stage."""
    R = rays_o.shape[0]
    S = int(sum(n_samples))
    dev = rays_o.device
    _chk(rays_o, torch.float32, "rays_o")
    _chk(rays_d, torch.float32, "rays_d")
    near = _chk(near.reshape(-1).contiguous(), torch.float32, "near")
    far = _chk(far.reshape(-1).contiguous(), torch.float32, "far")
    _chk(mvol, torch.float32, "matching volume")
    assert near.numel() == R and far.numel() == R
    if jitter is not None:
        _chk(jitter, torch.float32, "jitter")
        assert tuple(jitter.shape) == (R, len(n_samples)), jitter.shape
    lin_depth = _linspace_dev(0.0, 1.0, n_depth, dev)
    key = ("stages", tuple(int(n) for n in n_samples), str(dev))
    lin_s = _linspace_cache.get(key)
    if lin_s is None:
        lin_s = _linspace_cache[key] = torch.cat([torch.linspace(0.0, 1.0, int(n), dtype=torch.float32) for n in n_samples]).to(dev)
    out = {
        "mid_z": torch.empty(R, S, dtype=torch.float32, device=dev),
        "dists": torch.empty(R, S, dtype=torch.float32, device=dev),
        "pts": torch.empty(R * S, 3, dtype=torch.float32, device=dev),
        "vmask": torch.empty(R * S, dtype=torch.uint8, device=dev),
    }
    if want_z:
        out["z_vals"] = torch.empty(R, S, dtype=torch.float32, device=dev)
    ns = (ctypes.c_int * len(n_samples))(*[int(n) for n in n_samples])
    rg = (ctypes.c_float * len(sample_ranges))(*[float(r) for r in sample_ranges])
    _lib.lib().surf_ray_setup(_p(rays_o), _p(rays_d), _p(near), _p(far), R, _p(mvol), int(mvol.shape[-1]),
                              _p(lin_depth), int(n_depth), _p(lin_s), ns, rg, len(n_samples), _p(jitter),
                              float(2.0 / n_samples[0]), volumes._tp, volumes._dp, volumes.n,
                              _p(out.get("z_vals")), _p(out["mid_z"]), _p(out["dists"]), _p(out["pts"]),
                              _p(out["vmask"]), _stream())
    return out


_scratch_cache = {}


def _scratch(user, need, device):
    """A byte buffer of at least `need` bytes on `device`: one per user and device, replaced only by a larger one."""
    key = (user, device.index if device.index is not None else torch.cuda.current_device())
    buf = _scratch_cache.get(key)
    if buf is None or buf.numel() < need:
        buf = _scratch_cache[key] = torch.empty(need, dtype=torch.uint8, device=device)
    return buf


def _sdf_scratch(n, device, precision="f32"):
    fn = "surf_sdf_scratch_bytes" if precision == "f32" else f"surf_sdf_{_SPLIT_ABI[precision]}_scratch_bytes"
    return _scratch("sdf", getattr(_lib.lib(), fn)(int(n)), device)


def sdf_mlp(pts, volumes, packed, mask=None, want_grad=True, compact_active=True, active_idx=None, active_count=None):
    """sdf_network.py:95-141 at n points.  Returns (sdf (n,), grad (n,3) or None); masked-out rows are
    left at sdf=100 / grad=0 (what render_core substitutes, implicit_surface.py:93,99).
    active_count (with active_idx from compact_counted, split kernels only): the number of valid entries of active_idx as a
    DEVICE tensor - the kernel reads it there, no host sync."""
    _chk(pts, torch.float32, "pts")
    precision = sdf_packed_precision(packed)    # which kernel the packed weights were laid out for
    _chk(packed, torch.float32 if precision == "f32" else torch.uint8, "packed weights")
    n = pts.shape[0]
    dev = pts.device
    if mask is not None:
        _chk(mask, torch.uint8, "mask")
        sdf = torch.full((n,), 100.0, dtype=torch.float32, device=dev)
        grad = torch.zeros(n, 3, dtype=torch.float32, device=dev) if want_grad else None
    else:
        sdf = torch.empty(n, dtype=torch.float32, device=dev)
        grad = torch.empty(n, 3, dtype=torch.float32, device=dev) if want_grad else None
    idx, n_eval = None, n
    if active_idx is not None:
        idx, n_eval = active_idx, int(active_idx.shape[0])
        if n_eval == 0:
            return sdf, grad
    elif mask is not None and compact_active:
        idx = compact(mask)                 # wavefront tiles of active points only (one host sync for the count)
        n_eval = int(idx.shape[0])
        if n_eval == 0:
            return sdf, grad
    scratch = _sdf_scratch(n_eval, dev, precision) if want_grad else None
    name = {"f32": "surf_sdf_mlp", "bf16x3": "surf_sdf_mlp_bf16x3", "f16x2": "surf_sdf_mlp_f16x2"}[precision]
    if active_count is not None:
        if precision == "f32" or active_idx is None:
            raise ValueError("active_count needs active_idx and one of the split kernels (bf16x3 / f16x2)")
        _chk(active_count, torch.int32, "active_count")
        fn = getattr(_lib.lib(), name + "_dn")
        fn(_p(pts), _p(idx), n_eval, _p(active_count), volumes._vp, volumes._tp, volumes._dp, volumes.n, _p(packed), _p(sdf),
           _p(grad), _p(scratch), _stream())
        return sdf, grad
    fn = getattr(_lib.lib(), name)
    fn(_p(pts), _p(None if idx is not None else mask), _p(idx), n_eval, volumes._vp, volumes._tp, volumes._dp, volumes.n,
       _p(packed), _p(sdf), _p(grad), _p(scratch), _stream())
    return sdf, grad


def sdf_lattice(axes, volumes, packed, out, x0, nx, sign=-1.0):
    """out[x0:x0+nx] (a slab of the (X, Y, Z) lattice tensor `out`) = sign * sdf on the lattice axes[0][x0:x0+nx] x axes[1] x
    axes[2], by the forward-only split kernel in lattice mode (no point tensor: implicit_surface.py:337-351's meshgrid / cat
    is the kernel's index arithmetic).  Split precisions only."""
    precision = sdf_packed_precision(packed)
    if precision == "f32":
        raise ValueError("sdf_lattice: bf16x3 / f16x2 weights only (the fp32-MFMA kernel takes point tensors)")
    for ax in axes:
        _chk(ax, torch.float32, "lattice axis")
    _chk(out, torch.float32, "lattice values")
    ny, nz = int(axes[1].shape[0]), int(axes[2].shape[0])
    assert tuple(out.shape) == (int(axes[0].shape[0]), ny, nz) and 0 <= x0 and x0 + nx <= out.shape[0]
    name = f"surf_sdf_lattice_{precision}"
    getattr(_lib.lib(), name)(_p(axes[0][x0:]), _p(axes[1]), _p(axes[2]), int(nx), ny, nz, volumes._vp, volumes._tp, volumes._dp,
                              volumes.n, _p(packed), _p(out[x0:]), float(sign), _stream())


def sdf_smooth_pack_weights_host(layers):
    """[(W_l, b_l)] effective matrices -> fp32 image of the SDF network for surf_sdf_smooth (both orientations of every matrix)."""
    sdf_pack_weights_host(layers)  # shape validation only
    Ws = [_host_f32(W) for W, _ in layers]
    bs = [_host_f32(b) for _, b in layers]
    L = _lib.lib()
    out = np.zeros(L.surf_sdf_smooth_packed_floats(), dtype=np.float32)
    wp, bp = _host_ptr_array(Ws), _host_ptr_array(bs)
    L.surf_sdf_smooth_pack_weights(wp, bp, _np_ptr(out))
    return out


def sdf_smooth_pack_weights(sd, device, prefix="implicit_surface.sdf_network."):
    return torch.from_numpy(sdf_smooth_pack_weights_host(sdf_effective_weights(sd, prefix))).to(device)


def sdf_smooth(pts, volumes, packed, active_idx=None, want_grad=False):
    """sdf_network.py:143-152: smooth = d/dx sum_a (d sdf/d x_a) at n points.  Returns (smooth (n,3), grad (n,3) or
    None); rows not in active_idx stay zero (implicit_surface.py:100-103)."""
    _chk(pts, torch.float32, "pts")
    _chk(packed, torch.float32, "packed weights")
    n = pts.shape[0]
    if active_idx is not None:
        smooth = torch.zeros(n, 3, dtype=torch.float32, device=pts.device)
        grad = torch.zeros(n, 3, dtype=torch.float32, device=pts.device) if want_grad else None
        n_eval = int(active_idx.shape[0])
        if n_eval == 0:
            return smooth, grad
    else:
        smooth = torch.empty(n, 3, dtype=torch.float32, device=pts.device)
        grad = torch.empty(n, 3, dtype=torch.float32, device=pts.device) if want_grad else None
        n_eval = n
    _lib.lib().surf_sdf_smooth(_p(pts), _p(active_idx), n_eval, volumes._vp, volumes._tp, volumes._dp, volumes.n,
                               _p(packed), _p(grad), _p(smooth), _stream())
    return smooth, grad


def sdf_backward(pts, ybar, gbar, volumes, packed, want_dvols=True, dvols=None):
    """Gradients of sum_n (ybar_n sdf_n + gbar_n . grad_n) w.r.t. the EFFECTIVE (weight-normed) matrices / biases of
    lin0..lin6 and the sparse feature rows (surf_sdf_backward; the batch reductions dW = adj^T in are surf_colgram_p: matrix cores).
    packed: sdf_smooth_pack_weights.  Returns {"weight": [7 tensors shaped like W_l], "bias": [7], "volumes": [per level (N_s,8)]}."""
    _chk(pts, torch.float32, "pts")
    _chk(ybar, torch.float32, "ybar")
    _chk(gbar, torch.float32, "gbar")
    _chk(packed, torch.float32, "packed weights")
    n, dev = pts.shape[0], pts.device
    in_v = torch.empty(7, n, 160, dtype=torch.float32, device=dev)
    in_d = torch.empty(7, n, 160, dtype=torch.float32, device=dev)
    tb = torch.empty(6, n, 128, dtype=torch.float32, device=dev)
    tdb = torch.empty(6, n, 128, dtype=torch.float32, device=dev)
    if dvols is not None:       # rows to ACCUMULATE into (the kernel adds with atomics either way)
        assert len(dvols) == volumes.n and all(d.shape == v.shape and d.is_contiguous() for d, v in zip(dvols, volumes.vols))
    else:
        dvols = [torch.zeros_like(v) for v in volumes.vols] if want_dvols else None
    with _timed("sdf_bwd", n):
        _lib.lib().surf_sdf_backward(_p(pts), _p(ybar), _p(gbar), n, volumes._vp, volumes._tp, volumes._dp, volumes.n,
                                     _ptr_array(dvols) if dvols is not None else None, _p(packed), _p(in_v), _p(in_d), _p(tb),
                                     _p(tdb), _stream())
    shapes = [(128, 27), (128, 156), (101, 156), (128, 156), (128, 156), (128, 156), (129, 156)]
    dW, db = [], []
    for l in range(6):
        nl, kl = shapes[l]
        full = colgram(tb[l][:, :nl], in_v[l][:, :kl], with_sum=True)            # (N_l, K_l + 1): [tb^T in | sum tb]
        db.append(full[:, kl].contiguous())
        full = colgram(tdb[l][:, :nl], in_d[l][:, :kl], with_sum=True, out=full)  # + tdb^T in'   (its sum column is unused)
        dW.append(full[:, :kl].contiguous())
    w6 = torch.zeros(shapes[6], dtype=torch.float32, device=dev)                # only row 0 of lin6 reaches the loss
    w6[0] = (ybar[:, None] * in_v[6] + in_d[6]).sum(dim=0)[:156]
    b6 = torch.zeros(129, dtype=torch.float32, device=dev)
    b6[0] = ybar.sum()
    dW.append(w6)
    db.append(b6)
    return {"weight": dW, "bias": db, "volumes": dvols}


def sdf_smooth_backward(pts, sbar, volumes, packed, want_dvols=True, dvols=None):
    """Gradients of sum_n sbar_n . smooth_n (smooth = H.1 of the SDF, sdf_network.py:143-150) w.r.t. the EFFECTIVE matrices /
    biases of lin0..lin6 and the sparse feature rows (surf_sdf_smooth_backward; the batch reductions are surf_colgram).
    Returns the same dictionary as sdf_backward.  dvols: the (N_s, 8) gradient rows of an earlier sdf_backward to ACCUMULATE into
    (the kernel adds with atomics either way: saves a zero fill and a sum over ~10 M rows)."""
    _chk(pts, torch.float32, "pts")
    _chk(sbar, torch.float32, "sbar")
    _chk(packed, torch.float32, "packed weights")
    n, dev = pts.shape[0], pts.device
    xin = torch.empty(7, 4, n, 160, dtype=torch.float32, device=dev)
    ab = torch.empty(6, 4, n, 128, dtype=torch.float32, device=dev)
    if dvols is not None:
        assert len(dvols) == volumes.n and all(d.shape == v.shape and d.is_contiguous() for d, v in zip(dvols, volumes.vols))
    else:
        dvols = [torch.zeros_like(v) for v in volumes.vols] if want_dvols else None
    with _timed("sdf_smooth_bwd", n):
        _lib.lib().surf_sdf_smooth_backward(_p(pts), _p(sbar), n, volumes._vp, volumes._tp, volumes._dp, volumes.n,
                                            _ptr_array(dvols) if dvols is not None else None, _p(packed), _p(xin), _p(ab), _stream())
    shapes = [(128, 27), (128, 156), (101, 156), (128, 156), (128, 156), (128, 156), (129, 156)]
    dW, db = [], []
    for l in range(6):
        nl, kl = shapes[l]
        dW.append(colgram(ab[l].reshape(4 * n, 128)[:, :nl], xin[l].reshape(4 * n, 160)[:, :kl]))   # the four streams in one GEMM
        db.append(ab[l][0].sum(dim=0)[:nl].contiguous())
    w6 = torch.zeros(shapes[6], dtype=torch.float32, device=dev)                     # S = lin6 row 0 . (mixed input of lin6)
    w6[0] = xin[6][3].sum(dim=0)[:156]
    dW.append(w6)
    db.append(torch.zeros(129, dtype=torch.float32, device=dev))
    return {"weight": dW, "bias": db, "volumes": dvols}


# precision of the weight-gradient reductions (surf_colgram_p): 0 = fp32-equivalent, 1 = operands rounded to bf16 (fp32
# accumulate).  Set through `set_train_precision` (conf key `train_precision` of the model / bench --train-precision).
TRAIN_PRECISIONS = {"fp32": 0, "bf16": 1}
colgram_precision = 0
# thin sparse convolutions (a channel count of 8) on the matrix cores (csrc/spconv_mfma.hip, spconv_thin_mfma_kernel): "none"
# (default: the per-voxel FMA kernels of spconv.hip - both forms wait for the 27 row gathers of a site and the FMA form hides them
# better: profiles/r06_train_experiments.txt), "bf16" = under the bf16 training policy, "all" = also fp32-equivalent.  A/B switch.
thin_mfma = os.environ.get("SURF_THIN_MFMA", "none")
# bf16 ROW STORAGE of the sparse U-Net under the bf16 training policy (round 6): activations with 16 channels get a bf16 shadow
# (written by the BatchNorm apply / backward kernels in the same pass) that the (16 -> 8) thin convolutions gather from - the one
# channel pair where halving the row bytes pays (scripts/time_spconv_rows16.py: -35 .. -45 % per launch).  "0" = off (A/B switch).
layout_cache = os.environ.get("SURF_LAYOUT_CACHE", "1") != "0"   # FPN weight layouts cached per parameter version + the U-Nets' dgrad kernels built in the forward (A/B)
bf16_rows = os.environ.get("SURF_BF16_ROWS", "1") != "0"
bf16_rows_all_modes = os.environ.get("SURF_BF16_ROWS") == "all"      # also the stride-2 / transposed (16 -> 8) layers (measured: no gain)


def rows_to_bf16(x):
    """(n, C) fp32 rows -> their bf16 (round-to-nearest-even) bits as an (n, C) int16 tensor."""
    _chk(x, torch.float32, "x")
    out = torch.empty(x.shape, dtype=torch.int16, device=x.device)
    if x.numel():
        _lib.lib().surf_rows_to_bf16(_p(x), x.numel(), _p(out), _stream())
    return out


def set_train_precision(name):
    """Reduced-precision policy of the TRAINING step (BASELINE configs[3] "bf16").  "fp32" (default):
    every backward reduction fp32-equivalent.  "bf16": the operands of the weight-gradient reductions dW = adj^T in (the
    per-sample adjoint and input rows written by surf_sdf_backward / surf_sdf_smooth_backward / surf_blend_backward and the
    sparse U-Net's out_lin) are rounded to bf16 on load and multiplied on the matrix cores with fp32 accumulation.  Master
    weights, optimiser state, the adjoint propagation of the MLPs and every gather / scatter kernel stay fp32.  Round 5: the
    wide layers of the sparse U-Net (both channel counts >= 16, the matrix-core kernel) run their TRAINING forward and their
    input gradients on bf16-rounded operands too - one product per k-step instead of the exact split's six - which is what
    autocast(bf16) does to a convolution; the thin layers (gather bound) and the inference path are untouched."""
    global colgram_precision
    if name not in TRAIN_PRECISIONS:
        raise ValueError(f"train precision must be one of {sorted(TRAIN_PRECISIONS)}, got {name!r}")
    colgram_precision = TRAIN_PRECISIONS[name]
    return name


class precision_scope:
    """`with ops.precision_scope(p):` - run a BACKWARD under the training-precision policy its forward was recorded with
    (p = the value of `colgram_precision` then), whatever another model's forward has set since; restores the previous one."""

    def __init__(self, precision):
        self.precision = precision

    def __enter__(self):
        global colgram_precision
        self.saved = colgram_precision
        if self.precision is not None:
            colgram_precision = int(self.precision)

    def __exit__(self, *exc):
        global colgram_precision
        colgram_precision = self.saved
        return False


def colgram(A, X, with_sum=False, out=None, precision=None):
    """out (M, N [+1]) = A^T [X | 1] for row-major 2-D views A (rows, M), X (rows, N) that share contiguous rows (column
    slices of a wider buffer are fine: the row stride is taken from the view).  `out` given: accumulated into.
    precision: None = the module's training policy (`set_train_precision`), 0 = fp32-equivalent, 1 = bf16 operands."""
    assert A.dim() == 2 and X.dim() == 2 and A.shape[0] == X.shape[0] and A.stride(1) == 1 and X.stride(1) == 1
    assert A.dtype == torch.float32 and X.dtype == torch.float32 and A.is_cuda and X.is_cuda
    rows, M, N = int(A.shape[0]), int(A.shape[1]), int(X.shape[1])
    acc = out is not None
    if out is None:
        out = torch.empty(M, N + (1 if with_sum else 0), dtype=torch.float32, device=A.device)
    if rows == 0:
        return out if acc else out.zero_()
    ws = torch.empty(_lib.lib().surf_colgram_workspace_floats(rows, M, N), dtype=torch.float32, device=A.device)
    with _timed("colgram", rows * M * (N + (1 if with_sum else 0))):
        _lib.lib().surf_colgram_p(_p(A), int(A.stride(0)), M, _p(X), int(X.stride(0)), N, rows, int(with_sum), int(acc),
                                  int(colgram_precision if precision is None else precision), _p(ws), _p(out), _stream())
    return out


_BLEND_LAYERS = [  # (state_dict prefix, in, out, IN column, ADJ column) of surf_blend_backward's rows
    ("ray_dir_fc.0", 4, 16, 0, 4), ("ray_dir_fc.2", 16, 19, 20, 36), ("base_fc.0", 57, 64, 55, 112), ("base_fc.2", 64, 32, 176, 240),
    ("vis_fc.0", 32, 32, 272, 304), ("vis_fc.2", 32, 33, 336, 368), ("vis_fc2.0", 32, 32, 401, 433), ("vis_fc2.2", 32, 1, 465, 497),
    ("rgb_fc.0", 37, 16, 498, 535), ("rgb_fc.2", 16, 8, 551, 567), ("rgb_fc.4", 8, 1, 575, 583)]


def _check_blend_maps(feats_t4, imgs_t4, cams, gfeats_t4=None):
    """The blend kernels index the source images with the finest level's height and width and every map with cams.nv views,
    and take exactly four levels: anything else would read out of bounds, so it is refused before a launch."""
    if len(feats_t4) != 4:
        raise ValueError(f"blend: {len(feats_t4)} feature levels, the kernels take 4")
    for l, f in enumerate(feats_t4):
        if f.dim() != 4 or f.shape[3] != 4 or f.shape[0] != cams.nv:
            raise ValueError(f"blend: feature level {l} has shape {tuple(f.shape)}, expected ({cams.nv}, H, W, 4)")
    if tuple(imgs_t4.shape) != tuple(feats_t4[0].shape):
        raise ValueError(f"blend: imgs_t4 has shape {tuple(imgs_t4.shape)}, the finest feature level {tuple(feats_t4[0].shape)}")
    if gfeats_t4 is not None and [tuple(g.shape) for g in gfeats_t4] != [tuple(f.shape) for f in feats_t4]:
        raise ValueError("blend: gfeats_t4 must have the shapes of feats_t4")


def blend_backward(pts, active_idx, gcolor, feats_t4, imgs_t4, cams, raw_weights, want_color=False, gfeats_t4=None):
    """Gradients of sum_n gcolor_n . colour_n w.r.t. the blending network's parameters (surf_blend_backward; the batch
    reductions are surf_colgram_p: matrix cores).  raw_weights: device tensor of blend_raw_weights(sd) (packing.blend_raw_device).
    gfeats_t4: four texel4 maps shaped like feats_t4 that accumulate the gradient of the sampled feature channels.
    Returns {state_dict name: gradient} (+ "_color": the recomputed colours of the active samples, if asked)."""
    _check_blend_maps(feats_t4, imgs_t4, cams, gfeats_t4)
    _chk(pts, torch.float32, "pts")
    _chk(gcolor, torch.float32, "gcolor")
    _chk(raw_weights, torch.float32, "raw weights")
    assert gcolor.shape[0] == pts.shape[0]
    dev = pts.device
    n = int(active_idx.shape[0]) if active_idx is not None else pts.shape[0]
    V = cams.nv - 1
    ROW = _lib.lib().surf_blend_backward_row_floats()
    rows = torch.empty(max(n, 1), V, ROW, dtype=torch.float32, device=dev)
    ds = torch.zeros(max(n, 1), dtype=torch.float32, device=dev)
    color = torch.empty(max(n, 1), 3, dtype=torch.float32, device=dev) if want_color else None
    out = {}
    if n > 0:
        hw = (ctypes.c_int * 8)(*[int(v) for f in feats_t4 for v in f.shape[1:3]])
        intr16 = np.ascontiguousarray(cams.intrs.reshape(cams.nv, -1))
        with _timed("blend_bwd", n * V):
            _lib.lib().surf_blend_backward(_p(pts), _p(active_idx), n, _p(gcolor), _ptr_array(list(feats_t4)), hw, _p(imgs_t4),
                                           cams.nv, _np_ptr(intr16), _np_ptr(cams.w2c), _np_ptr(cams.c2w), _p(raw_weights),
                                           _p(rows), _p(ds), _p(color),
                                           None if gfeats_t4 is None else _ptr_array(list(gfeats_t4)), _stream())
    flat = rows[:n].reshape(-1, ROW)
    for name, cin, cout, c_in, c_ad in _BLEND_LAYERS:
        g = colgram(flat[:, c_ad:c_ad + cout], flat[:, c_in:c_in + cin], with_sum=True)
        out[name + ".weight"] = g[:, :cin].contiguous()
        out[name + ".bias"] = g[:, cin].contiguous()
    out["s"] = ds[:n].sum().reshape(())
    if want_color:
        out["_color"] = color[:n]
    return out


class Cameras:
    """Host copies of the 4x4 camera matrices the kernels take by value."""

    def __init__(self, intrs, c2ws):
        self.nv = int(intrs.shape[0])
        c2w_cpu = c2ws.detach().to("cpu", torch.float32)
        self.intrs = np.ascontiguousarray(intrs.detach().to("cpu", torch.float32).numpy())
        self.c2w = np.ascontiguousarray(c2w_cpu.numpy())
        self.w2c = np.ascontiguousarray(torch.inverse(c2w_cpu).numpy())
        self.rot_ref = np.ascontiguousarray(torch.inverse(c2w_cpu[0, :3, :3]).numpy())


def blend(pts, feats_t4, imgs_t4, cams, packed, mask=None, compact_active=True, active_idx=None, active_count=None):
    """projector.py:501-556 + blending_network.py:69-118.  feats_t4: list fine -> coarse of (nv,H,W,4).
    Returns (color (n,3), n_valid (n) uint8); masked-out rows are zero."""
    _check_blend_maps(feats_t4, imgs_t4, cams)
    _chk(pts, torch.float32, "pts")
    n = pts.shape[0]
    dev = pts.device
    for f in feats_t4:
        _chk(f, torch.float32, "feature map")
    _chk(imgs_t4, torch.float32, "imgs")
    color = torch.zeros(n, 3, dtype=torch.float32, device=dev)
    nvalid = torch.zeros(n, dtype=torch.uint8, device=dev)
    hw = (ctypes.c_int * (2 * len(feats_t4)))(*[int(v) for f in feats_t4 for v in f.shape[1:3]])
    fp = _ptr_array(feats_t4)
    idx, n_eval = None, n
    if active_idx is not None:
        idx, n_eval = active_idx, int(active_idx.shape[0])
    elif mask is not None and compact_active:
        idx = compact(mask)
        n_eval = int(idx.shape[0])
    if n_eval == 0:
        return color, nvalid
    precision = blend_packed_precision(packed)     # which kernel the packed weights were laid out for
    if precision == "f32" and active_count is not None:
        raise ValueError("active_count needs one of the split blend kernels")
    if precision == "f32":
        _lib.lib().surf_blend(_p(pts), _p(None if idx is not None else mask), _p(idx), n_eval, fp, hw, len(feats_t4),
                              _p(imgs_t4), cams.nv, _np_ptr(cams.intrs), _np_ptr(cams.w2c), _np_ptr(cams.c2w), _p(packed),
                              _p(color), _p(nvalid), _stream())
    else:
        scratch = _scratch("blend", _lib.lib().surf_blend_split_scratch_bytes(int(n_eval), cams.nv), dev)
        if active_count is not None:           # the count stays on the device (compact_counted)
            _chk(active_count, torch.int32, "active_count")
            _lib.lib().surf_blend_split_dn(_p(pts), _p(idx), n_eval, _p(active_count), fp, hw, len(feats_t4), _p(imgs_t4),
                                           cams.nv, _np_ptr(cams.intrs), _np_ptr(cams.w2c), _np_ptr(cams.c2w), _p(packed),
                                           _BLEND_ID[precision], _p(color), _p(nvalid), _p(scratch), _stream())
        else:
            _lib.lib().surf_blend_split(_p(pts), _p(None if idx is not None else mask), _p(idx), n_eval, fp, hw, len(feats_t4),
                                        _p(imgs_t4), cams.nv, _np_ptr(cams.intrs), _np_ptr(cams.w2c), _np_ptr(cams.c2w),
                                        _p(packed), _BLEND_ID[precision], _p(color), _p(nvalid), _p(scratch), _stream())
    return color, nvalid


def composite(sdf, grad, color, n_valid, setup, rays_d, inv_s, cos_anneal_ratio, cams, per_sample=True, want_z0=False):
    """implicit_surface.py:126-166,181-216.  Returns the per-ray dict (+ weights / inside_sphere if per_sample;
    + z_sdf0, the zero crossing's ray parameter, if want_z0)."""
    R, S = setup["mid_z"].shape
    dev = sdf.device
    f32 = dict(dtype=torch.float32, device=dev)
    out = {
        "color_fine": torch.empty(R, 3, **f32), "render_depth": torch.empty(R, **f32),
        "sdf_depth": torch.empty(R, 1, **f32), "normal": torch.empty(R, 3, **f32),
        "normal_val": torch.empty(R, 3, **f32), "valid_mask": torch.empty(R, 1, dtype=torch.uint8, device=dev),
        "mid_inside_sphere": torch.empty(R, 1, dtype=torch.uint8, device=dev), "eik": torch.empty(R, 2, **f32),
    }
    if per_sample:
        out["weights"] = torch.empty(R, S, **f32)
        out["inside_sphere"] = torch.empty(R, S, **f32)
    if want_z0:
        out["z_sdf0"] = torch.empty(R, **f32)
    _lib.lib().surf_composite(_p(sdf), _p(grad), _p(color), _p(n_valid), _p(setup["mid_z"]), _p(setup["dists"]),
                              _p(setup["pts"]), _p(setup["vmask"]), _p(rays_d), R, S, float(inv_s),
                              float(cos_anneal_ratio), _np_ptr(cams.rot_ref), _p(out["color_fine"]),
                              _p(out["render_depth"]), _p(out["sdf_depth"]), _p(out["normal"]),
                              _p(out["normal_val"]), _p(out["valid_mask"]), _p(out["mid_inside_sphere"]),
                              _p(out.get("weights")), _p(out.get("inside_sphere")), _p(out["eik"]), _p(out.get("z_sdf0")),
                              _stream())
    return out


def composite_backward(sdf, grad, color, setup, rays_d, inv_s, cos_anneal_ratio, cams, g_color, g_depth=None, eik_scale=0.0,
                       eik_upstream=None):
    """Backward of `composite` w.r.t. (sdf, grad, color, inv_s) for upstream gradients of colour_fine (R,3) and
    render_depth (R) and the eikonal term (eik_scale = dL/d gradient_error / (sum relax + 1e-5)).
    Returns (d_sdf (R*S,), d_grad (R*S,3), d_color (R*S,3), d_inv_s scalar tensor)."""
    R, S = setup["mid_z"].shape
    dev = sdf.device
    _chk(g_color, torch.float32, "g_color")
    d_sdf = torch.empty(R * S, dtype=torch.float32, device=dev)
    d_grad = torch.empty(R * S, 3, dtype=torch.float32, device=dev)
    d_color = torch.empty(R * S, 3, dtype=torch.float32, device=dev)
    d_is = torch.empty(R, dtype=torch.float32, device=dev)
    if eik_upstream is not None:        # dL/d gradient_error as a device scalar: multiplied in inside the kernel, never read back
        eik_upstream = _chk(eik_upstream.detach().reshape(1).float().contiguous(), torch.float32, "eik_upstream")
    _lib.lib().surf_composite_backward_s(_p(sdf), _p(grad), _p(color), _p(setup["mid_z"]), _p(setup["dists"]), _p(setup["pts"]),
                                         _p(setup["vmask"]), _p(rays_d), R, S, float(inv_s),
                                         float(cos_anneal_ratio), _np_ptr(cams.rot_ref), _p(g_color), _p(g_depth),
                                         float(eik_scale), _p(eik_upstream), _p(d_sdf), _p(d_grad), _p(d_color),
                                         _p(d_is), _stream())
    return d_sdf, d_grad, d_color, d_is.sum(dtype=torch.float64).float()


def upsample_bilinear_t4(x, H, W):
    """F.interpolate(x, size=(H, W), mode="bilinear", align_corners=False) on a texel4 map (n,h,w,4)."""
    _chk(x, torch.float32, "x")
    n, h, w, c = x.shape
    assert c == 4
    out = torch.empty(n, H, W, 4, dtype=torch.float32, device=x.device)
    _lib.lib().surf_upsample_bilinear_t4(_p(x), n, h, w, int(H), int(W), _p(out), _stream())
    return out


def surface_points(rays_o, rays_d, z_sdf0, z_vals):
    """implicit_surface.py:217-220: the zero crossing's ray parameter zeroed outside [0, max(z_vals)], then o + d z."""
    _chk(rays_o, torch.float32, "rays_o")
    _chk(rays_d, torch.float32, "rays_d")
    _chk(z_sdf0, torch.float32, "z_sdf0")
    _chk(z_vals, torch.float32, "z_vals")
    R = rays_o.shape[0]
    ws = torch.empty(1, dtype=torch.int32, device=rays_o.device)
    pts = torch.empty(R, 3, dtype=torch.float32, device=rays_o.device)
    _lib.lib().surf_surface_points(_p(rays_o), _p(rays_d), _p(z_sdf0), R, _p(z_vals), z_vals.numel(), _p(ws), _p(pts), _stream())
    return pts


def patch_warp(pts, grads, maps_t4, cams, patch_size=11):
    """projector.py:560-645 (+ the normal's normalisation and rotation of implicit_surface.py:224-228).
    maps_t4: the three finest feature levels as texel4 (nv,H,W,4) at full resolution; cams: ops.Cameras.
    Returns (ref_gray_val (1,R,p*p,12), sampled_gray_val (nv-1,R,p*p,12))."""
    _chk(pts, torch.float32, "pts")
    _chk(grads, torch.float32, "grads")
    for m in maps_t4:
        _chk(m, torch.float32, "feature map")
    nv, H, W, _ = maps_t4[0].shape
    assert len(maps_t4) == 3 and all(tuple(m.shape) == (nv, H, W, 4) for m in maps_t4)
    R = pts.shape[0]
    dev = pts.device
    if not hasattr(cams, "kinv_ref"):
        cams.kinv_ref = np.ascontiguousarray(torch.inverse(torch.from_numpy(cams.intrs))[0, :3, :3].contiguous().numpy())
    K, kinv, c2w = cams.intrs, cams.kinv_ref, cams.c2w
    assert cams.nv == nv
    P = patch_size * patch_size
    ref = torch.empty(1, R, P, 12, dtype=torch.float32, device=dev)
    src = torch.empty(nv - 1, R, P, 12, dtype=torch.float32, device=dev)
    _lib.lib().surf_patch_warp(_p(pts), _p(grads), R, _ptr_array(list(maps_t4)), nv, H, W, _np_ptr(K), _np_ptr(kinv),
                               _np_ptr(c2w), int(patch_size), _p(ref), _p(src), _stream())
    return ref, src


def photometric_loss(depth, imgs_t4, mask_ref, cams, ref_idx=0, topk=2, return_warp=False, return_state=False, return_terms=False):
    """compute_ptloss (losses/photometric_loss.py:54-125) of one (H,W) depth map of view ref_idx: scalar tensor.
    imgs_t4 (nv,H,W,4) texel4; cams: ops.Cameras (host matrices).  return_state: (loss, (warp, column sums)) - what
    photometric_loss_backward would otherwise recompute with a second run of the forward kernel.  return_terms: (loss, warp,
    terms) with the per-pixel (H,W,8) columns [l1 m, gx mx, gy my, ssim m | m, mx, my, m] the scalar is reduced from."""
    _chk(depth, torch.float32, "depth")
    _chk(imgs_t4, torch.float32, "imgs_t4")
    _chk(mask_ref, torch.float32, "mask_ref")
    nv, H, W, _ = imgs_t4.shape
    assert tuple(depth.shape) == (H, W) and tuple(mask_ref.shape) == (H, W) and cams.nv == nv
    dev = depth.device
    warp = torch.empty(nv - 1, H, W, 4, dtype=torch.float32, device=dev)
    terms = torch.empty(H, W, 8, dtype=torch.float32, device=dev)
    intr16 = np.ascontiguousarray(cams.intrs.reshape(nv, -1))
    assert intr16.shape[1] == 16
    _lib.lib().surf_ptloss_terms(_p(imgs_t4), nv, H, W, _p(depth), _p(mask_ref), int(ref_idx), int(topk), _np_ptr(intr16),
                                 _np_ptr(cams.c2w), _np_ptr(cams.w2c), _p(warp), _p(terms), _stream())
    t = terms.view(-1, 8).sum(dim=0, dtype=torch.float64)       # columns [l1 m, gx mx, gy my, ssim m | m, mx, my, m]
    loss = (t[:4] / (t[4:] + 1e-8)).sum().float()
    if return_terms:
        return loss, warp, terms
    if return_state:
        return loss, (warp, t)
    return (loss, warp) if return_warp else loss


def photometric_loss_backward(depth, imgs_t4, mask_ref, cams, ref_idx=0, topk=2, upstream=1.0, state=None):
    """d (upstream * photometric_loss(depth, ...)) / d depth (H,W) (surf_ptloss_backward).  state: the forward's (warp, column
    sums) (photometric_loss(..., return_state=True)); None: the forward kernel is re-run for them.  upstream: float or 0-d
    device tensor."""
    _chk(depth, torch.float32, "depth")
    nv, H, W, _ = imgs_t4.shape
    dev = depth.device
    intr16 = np.ascontiguousarray(cams.intrs.reshape(nv, -1))
    if state is not None:
        warp, t = state
    else:
        warp = torch.empty(nv - 1, H, W, 4, dtype=torch.float32, device=dev)
        terms = torch.empty(H, W, 8, dtype=torch.float32, device=dev)
        _lib.lib().surf_ptloss_terms(_p(imgs_t4), nv, H, W, _p(depth), _p(mask_ref), int(ref_idx), int(topk), _np_ptr(intr16),
                                     _np_ptr(cams.c2w), _np_ptr(cams.w2c), _p(warp), _p(terms), _stream())
        t = terms.view(-1, 8).sum(dim=0, dtype=torch.float64)
    coef = (upstream / (t[4:] + 1e-8)).float().contiguous()
    g_warp = torch.empty_like(warp)
    g_depth = torch.empty(H, W, dtype=torch.float32, device=dev)
    _lib.lib().surf_ptloss_backward(_p(imgs_t4), nv, H, W, _p(depth), _p(mask_ref), int(ref_idx), int(topk), _np_ptr(intr16),
                                    _np_ptr(cams.c2w), _np_ptr(cams.w2c), _p(warp), _p(coef), _p(g_warp), _p(g_depth), _stream())
    return g_depth


def patch_warp_tangent(pts, dirs, grads, maps_t4, cams, patch_size=11):
    """patch_warp + the derivatives of both patch stacks along d pts / d z0 = dirs (R,3) (surf_patch_warp_tangent).
    Returns (ref, src, ref_tan, src_tan)."""
    for t, nm in ((pts, "pts"), (dirs, "dirs"), (grads, "grads")):
        _chk(t, torch.float32, nm)
    nv, H, W, _ = maps_t4[0].shape
    R, dev, P = pts.shape[0], pts.device, patch_size * patch_size
    if not hasattr(cams, "kinv_ref"):
        cams.kinv_ref = np.ascontiguousarray(torch.inverse(torch.from_numpy(cams.intrs))[0, :3, :3].contiguous().numpy())
    ref, ref_t = (torch.empty(1, R, P, 12, dtype=torch.float32, device=dev) for _ in range(2))
    src, src_t = (torch.empty(nv - 1, R, P, 12, dtype=torch.float32, device=dev) for _ in range(2))
    _lib.lib().surf_patch_warp_tangent(_p(pts), _p(dirs), _p(grads), R, _ptr_array(list(maps_t4)), nv, H, W, _np_ptr(cams.intrs),
                                       _np_ptr(cams.kinv_ref), _np_ptr(cams.c2w), int(patch_size), _p(ref), _p(src), _p(ref_t),
                                       _p(src_t), _stream())
    return ref, src, ref_t, src_t


def lncc_jvp(ref, src, ref_tan, src_tan):
    """(ncc (R,1), d ncc / d z0 (R,)) of compute_LNCC2 for patch tangents (surf_lncc_jvp)."""
    nsrc, R, P, C = src.shape
    ncc = torch.empty(R, 1, dtype=torch.float32, device=ref.device)
    d = torch.empty(R, dtype=torch.float32, device=ref.device)
    _lib.lib().surf_lncc_jvp(_p(ref), _p(src), _p(ref_tan), _p(src_tan), R, int(nsrc), int(P), int(C), _p(ncc), _p(d), _stream())
    return ncc, d


def crossing_backward(sdf, vmask, mid_z, zmax, g_z0, d_sdf):
    """d_sdf (R*S,) += g_z0 (R,) d z0 / d sdf at the first zero crossing of every ray (surf_crossing_backward); zmax: 0-d tensor."""
    R, S = mid_z.shape
    _chk(d_sdf, torch.float32, "d_sdf")
    _lib.lib().surf_crossing_backward(_p(sdf), _p(vmask), _p(mid_z), R, S, _p(zmax.reshape(1).float().contiguous()),
                                      _p(g_z0.float().contiguous()), _p(d_sdf), _stream())
    return d_sdf


def lncc(ref_gray_val, sampled_gray_val):
    """compute_LNCC2 (losses/ncc.py:7-51): ref (1,R,P,C), src (nsrc,R,P,C) -> (R,1)."""
    _chk(ref_gray_val, torch.float32, "ref_gray_val")
    _chk(sampled_gray_val, torch.float32, "sampled_gray_val")
    nsrc, R, P, C = sampled_gray_val.shape
    assert tuple(ref_gray_val.shape) == (1, R, P, C)
    out = torch.empty(R, 1, dtype=torch.float32, device=ref_gray_val.device)
    if R > 0:
        _lib.lib().surf_lncc(_p(ref_gray_val), _p(sampled_gray_val), R, int(nsrc), int(P), int(C), _p(out), _stream())
    return out


def lncc_backward(ref_gray_val, sampled_gray_val, g_ncc):
    """(d/d ref_gray_val, d/d sampled_gray_val) of sum_r g_ncc[r] * compute_LNCC2(ref, src)[r] (surf_lncc_backward)."""
    _chk(ref_gray_val, torch.float32, "ref_gray_val")
    _chk(sampled_gray_val, torch.float32, "sampled_gray_val")
    nsrc, R, P, C = sampled_gray_val.shape
    g = _chk(g_ncc.reshape(-1).float().contiguous(), torch.float32, "g_ncc")
    assert g.shape[0] == R
    g_ref, g_src = torch.empty_like(ref_gray_val), torch.empty_like(sampled_gray_val)
    if R > 0:
        _lib.lib().surf_lncc_backward(_p(ref_gray_val), _p(sampled_gray_val), _p(g), R, int(nsrc), int(P), int(C),
                                      _p(g_ref), _p(g_src), _stream())
    return g_ref, g_src


# ------------------------------------------------------------------------------------------------
# volume build (surf.py:80-131)
# ------------------------------------------------------------------------------------------------


def _cams_ext(cams, intrs, c2ws):
    """Extra host matrices of the matching field: inverse(intrs)[:, :3, :3], inverse(c2w[:, :3, :3])."""
    if not hasattr(cams, "kinv"):
        i_cpu = intrs.detach().to("cpu", torch.float32)
        c_cpu = c2ws.detach().to("cpu", torch.float32)
        cams.kinv = np.ascontiguousarray(torch.inverse(i_cpu)[:, :3, :3].contiguous().numpy())
        cams.rinv = np.ascontiguousarray(torch.inverse(c_cpu[:, :3, :3]).contiguous().numpy())
    return cams


def upsample_filter(parents, D, depths, cams, depth_range):
    """volume.py:35-52 + 134-165: flags (8 N,) uint8 over the children of `parents` (N,3) int32."""
    _chk(parents, torch.int32, "parents")
    _chk(depths, torch.float32, "depths")
    nv, H, W = depths.shape
    flags = torch.empty(parents.shape[0] * 8, dtype=torch.uint8, device=parents.device)
    _lib.lib().surf_upsample_filter(_p(parents), parents.shape[0], int(D), _p(depths), nv, H, W, _np_ptr(cams.intrs),
                                    _np_ptr(cams.w2c), float(depth_range), _p(flags), _stream())
    return flags


def agg_mlp_host(sd, prefix="volume."):
    return np.concatenate([_host_f32(sd[prefix + k]).reshape(-1) for k in
                           ("agg_mlp.0.weight", "agg_mlp.0.bias", "agg_mlp.2.weight", "agg_mlp.2.bias")])


def costvol(feats_t4_c2f, stage, D, cams, agg, parents=None, idx=None):
    """volume.py:54-97 on the full lattice (parents/idx None) or on children idx of parents.
    feats_t4_c2f: texel4 pyramids coarse -> fine.  Returns coords (n,3) int32, feat (n,8), keep (n,) uint8."""
    dev = feats_t4_c2f[0].device
    n = int(D) ** 3 if idx is None else int(idx.shape[0])
    coords = torch.empty(n, 3, dtype=torch.int32, device=dev)
    feat = torch.empty(n, 8, dtype=torch.float32, device=dev)
    keep = torch.empty(n, dtype=torch.uint8, device=dev)
    hw = (ctypes.c_int * 8)(*[int(v) for f in feats_t4_c2f for v in f.shape[1:3]])
    fp = _ptr_array(feats_t4_c2f)
    agg = np.ascontiguousarray(agg, dtype=np.float32)
    _lib.lib().surf_costvol(_p(parents), _p(idx), n, int(D), fp, hw, int(stage), cams.nv, _np_ptr(cams.intrs),
                            _np_ptr(cams.w2c), _np_ptr(agg), _p(coords), _p(feat), _p(keep), _stream())
    return coords, feat, keep


def compact(flags):
    """Ascending indices of the set flags (int32).  One host sync to size the result -- the reference syncs at the
    same places (boolean-mask indexing, volume.py:165-166, surf.py:104-108)."""
    _chk(flags, torch.uint8, "flags")
    n = flags.numel()
    dev = flags.device
    ws = torch.empty(_lib.lib().surf_compact_workspace_ints(n), dtype=torch.int32, device=dev)
    idx = torch.empty(n, dtype=torch.int32, device=dev)
    total = torch.empty(1, dtype=torch.int32, device=dev)
    _lib.lib().surf_compact(_p(flags), n, _p(ws), _p(idx), _p(total), _stream())
    return idx[:int(total.item())]


def compact_counted(flags, block=None):
    """compact without the host round trip: (idx (n,) int32 of which the first `count` entries are the ascending indices of
    the set flags, count (1,) int32 ON THE DEVICE).  For consumers that read the count from device memory (sdf_mlp / blend
    with `active_count`).
    block = (S, G, B): the flags are an (n / S, S) ray-major array and the same indices come in the traversal order
    (ray // G, s // B, ray % G, s % B) - blocks of G neighbouring rays by B consecutive samples (surf_compact_blocked;
    G and B powers of two, B divides S) - instead of ascending."""
    _chk(flags, torch.uint8, "flags")
    n = flags.numel()
    dev = flags.device
    ws = torch.empty(_lib.lib().surf_compact_workspace_ints(n), dtype=torch.int32, device=dev)
    idx = torch.empty(n, dtype=torch.int32, device=dev)
    total = torch.empty(1, dtype=torch.int32, device=dev)
    if block is None:
        _lib.lib().surf_compact(_p(flags), n, _p(ws), _p(idx), _p(total), _stream())
    else:
        S, G, B = (int(v) for v in block)
        if S <= 0 or n % S:
            raise ValueError(f"compact_counted: {n} flags are no whole number of rays of {S} samples")
        _lib.lib().surf_compact_blocked(_p(flags), n // S, S, G, B, _p(ws), _p(idx), _p(total), _stream())
    return idx, total


def gather_rows(src, idx, shift=0, dst=None, dst_off=0):
    """dst[i, off:off+w] = src[idx[i] >> shift]; src rows of 32-bit elements."""
    assert src.is_contiguous() and src.element_size() == 4 and src.is_cuda
    _chk(idx, torch.int32, "idx")
    w = src.shape[1]
    n = idx.shape[0]
    if dst is None:
        dst = torch.empty(n, w, dtype=src.dtype, device=src.device)
    _lib.lib().surf_gather_rows(_p(src), _p(idx), n, w, int(shift), dst.shape[1], int(dst_off), _p(dst), _stream())
    return dst


def compose_index(a, b):
    out = torch.empty_like(b)
    _lib.lib().surf_compose_index(_p(a), _p(b), b.shape[0], _p(out), _stream())
    return out


def densify(coords, rows, D, prev=None):
    """volume.py:99-132: dense matching volume (D,D,D) f32 and index table (D,D,D) int32; logit = rows[:, 0]."""
    _chk(coords, torch.int32, "coords")
    _chk(rows, torch.float32, "rows")
    dev = coords.device
    dense = torch.empty(D, D, D, dtype=torch.float32, device=dev)
    table = torch.empty(D, D, D, dtype=torch.int32, device=dev)
    _lib.lib().surf_densify(_p(coords), _p(rows), rows.shape[1], coords.shape[0], int(D), _p(prev), _p(dense), _p(table), _stream())
    return dense, table


def matching_depth(mvol, cams, near_fars, H, W, res_level, n, pre_depths=None, ratio_cur=1.0, ratio_prev=1.0, return_lr=False,
                   jitter=None, saved=None):
    """matching_field.py:73-141.  Returns depth maps (nv,H,W) (and, with return_lr, the (nv,h,w) maps rendered at the
    reduced resolution before the bilinear upsample).  jitter (nv, h*w, 2): the train-mode per-ray, per-band z shifts.
    saved: a dict that receives "stats" (nv,h,w,4) = the per-ray softmax statistics matching_depth_backward can start from."""
    _chk(mvol, torch.float32, "matching volume")
    dev = mvol.device
    h, w = H // res_level, W // res_level
    lin_x = _linspace_dev(0, W - 1, w, dev)
    lin_y = _linspace_dev(0, H - 1, h, dev)
    lin_n = _linspace_dev(0.0, 1.0, n, dev)
    nf = _near_fars_host(near_fars)
    lr = torch.empty(cams.nv, h, w, dtype=torch.float32, device=dev)
    full = torch.empty(cams.nv, H, W, dtype=torch.float32, device=dev)
    if jitter is not None:
        _chk(jitter, torch.float32, "jitter")
        assert tuple(jitter.shape) == (cams.nv, h * w, 2)
    stats = torch.empty(cams.nv, h, w, 4, dtype=torch.float32, device=dev) if saved is not None else None
    _lib.lib().surf_matching_depth(_p(mvol), int(mvol.shape[0]), cams.nv, _np_ptr(cams.kinv), _np_ptr(cams.c2w),
                                   _np_ptr(cams.rinv), _np_ptr(nf), H, W, h, w, _p(lin_x), _p(lin_y), _p(lin_n), int(n),
                                   _p(pre_depths), float(ratio_cur), float(ratio_prev),
                                   _p(jitter), _p(lr), _p(full), _p(stats), _stream())
    if saved is not None:
        saved["stats"] = stats
    return (full, lr) if return_lr else full


def matching_depth_backward(mvol, cams, near_fars, H, W, res_level, n, g_full, pre_depths=None, ratio_cur=1.0, ratio_prev=1.0,
                            jitter=None, dmvol=None, views=(0, 0), stats=None):
    """Backward of matching_depth w.r.t. the matching volume: g_full (nv,H,W) = d loss / d depth maps; only the maps of
    `views` = (reference view, src_idx) are read (the reference renders the others under no_grad).  Returns dmvol (D,D,D),
    accumulated into `dmvol` if given.  stats: the forward's per-ray softmax statistics (matching_depth(..., saved=)) for the SAME
    arguments and jitter - the kernel then walks the samples once instead of twice."""
    _chk(mvol, torch.float32, "matching volume")
    _chk(g_full, torch.float32, "g_full")
    dev = mvol.device
    h, w = H // res_level, W // res_level
    assert tuple(g_full.shape) == (cams.nv, H, W)
    lin_x = _linspace_dev(0, W - 1, w, dev)
    lin_y = _linspace_dev(0, H - 1, h, dev)
    lin_n = _linspace_dev(0.0, 1.0, n, dev)
    nf = _near_fars_host(near_fars)
    g_lr = torch.empty(cams.nv, h, w, dtype=torch.float32, device=dev)
    if stats is not None:
        _chk(stats, torch.float32, "stats")
        assert tuple(stats.shape) == (cams.nv, h, w, 4)
    if dmvol is None:
        dmvol = torch.zeros_like(mvol)
    n_views = len(set(int(v) for v in views))
    with _timed("matching_depth_bwd", n_views * h * w * int(n) * (1 if pre_depths is None else 2)):
        _lib.lib().surf_matching_depth_backward(_p(mvol), int(mvol.shape[0]), cams.nv, _np_ptr(cams.kinv), _np_ptr(cams.c2w),
                                                _np_ptr(cams.rinv), _np_ptr(nf), H, W, h, w, _p(lin_x), _p(lin_y), _p(lin_n),
                                                int(n), _p(pre_depths), float(ratio_cur),
                                                float(ratio_prev), _p(jitter), _p(g_full), int(views[0]), int(views[1]),
                                                _p(g_lr), _p(dmvol), _p(stats), _stream())
    return dmvol


def densify_backward(coords, table, g_dense, g_rows, g_prev=None):
    """Backward of densify: g_rows[:, 0] += g_dense[coords]; g_prev (D/2)^3 (if given) accumulates the background's share."""
    _chk(coords, torch.int32, "coords")
    _chk(g_dense, torch.float32, "g_dense")
    _chk(g_rows, torch.float32, "g_rows")
    D = int(g_dense.shape[0])
    _lib.lib().surf_densify_backward(_p(coords), coords.shape[0], D, _p(table), _p(g_dense), g_rows.shape[1], _p(g_rows),
                                     _p(g_prev), _stream())
    return g_rows, g_prev


def scatter_rows_add(g_dst, idx, g_src, shift=0, dst_off=0):
    """Backward of gather_rows: g_src[idx[i] >> shift] += g_dst[i, off : off + w], w = g_src.shape[1]."""
    _chk(g_dst, torch.float32, "g_dst")
    _chk(g_src, torch.float32, "g_src")
    _chk(idx, torch.int32, "idx")
    _lib.lib().surf_scatter_rows_add(_p(g_dst), _p(idx), idx.shape[0], g_src.shape[1], int(shift), g_dst.shape[1],
                                     int(dst_off), _p(g_src), _stream())
    return g_src


def costvol_backward(feats_t4_c2f, gfeats_t4_c2f, stage, D, cams, agg, coords, g, g_agg):
    """Backward of costvol for the kept voxels: accumulates into gfeats_t4_c2f[l] (l >= stage) and g_agg (49,)."""
    _chk(coords, torch.int32, "coords")
    _chk(g, torch.float32, "g")
    _chk(g_agg, torch.float32, "g_agg")
    assert g.shape[1] == 8 and g_agg.numel() == 49
    hw = (ctypes.c_int * 8)(*[int(v) for f in feats_t4_c2f for v in f.shape[1:3]])
    agg = np.ascontiguousarray(agg, dtype=np.float32)
    # 9 floats per (view, voxel) pair when the tile-sorted form runs (1.1 - 1.5 GB at the finest DTU stage), 4,096 floats otherwise
    ws = torch.empty(_lib.lib().surf_costvol_backward_workspace_floats_for(coords.shape[0], cams.nv, hw),
                     dtype=torch.float32, device=g.device)
    with _timed("costvol_bwd", int(coords.shape[0]) * cams.nv * (4 - int(stage))):
        _lib.lib().surf_costvol_backward(_p(coords), _p(g), coords.shape[0], int(D), _ptr_array(feats_t4_c2f),
                                         _ptr_array(gfeats_t4_c2f), hw, int(stage), cams.nv, _np_ptr(cams.intrs),
                                         _np_ptr(cams.w2c), _np_ptr(agg), _p(ws), _p(g_agg), _stream())


def raster_first_hit(vertices, faces, intr, c2w, hw, upscale=1):
    """Face id of the first triangle hit by the ray through every sample of the (h*upscale, w*upscale) lattice
    torch.linspace(0, w-1, w*upscale) x torch.linspace(0, h-1, h*upscale) of one view; -1 where nothing is hit."""
    _chk(vertices, torch.float32, "vertices")
    _chk(faces, torch.int32, "faces")
    h, w = int(hw[0]), int(hw[1])
    Hup, Wup = int(h * upscale), int(w * upscale)
    K = np.ascontiguousarray(intr.detach().to("cpu", torch.float32)[:3, :3].contiguous().numpy())
    w2c = np.ascontiguousarray(torch.inverse(c2w.detach().to("cpu", torch.float32))[:3, :4].contiguous().numpy())
    zbuf = torch.full((Hup, Wup), -1, dtype=torch.int64, device=vertices.device)      # all ones = empty
    _lib.lib().surf_raster_first_hit(_p(vertices), _p(faces), faces.shape[0], _np_ptr(K), _np_ptr(w2c), h, w, Hup, Wup,
                                     _p(zbuf), _stream())
    return torch.where(zbuf == -1, torch.full_like(zbuf, -1), zbuf & 0xffffffff)


def raster_depth(vertices, faces, P, hw):
    """The z-buffer of a mesh from the camera P (3, 4) fp32 on the host (world -> (x z, y z, z) in pixel indices): (H, W) fp32,
    the depth of the nearest face at every pixel, 0 where nothing is hit.  surf_raster_first_hit in P's own pixel units (K = I,
    w2c = P, one sample per pixel): the depth raster_first_hit throws away, the upper 32 bits of the keys.  No faces: all 0."""
    _chk(vertices, torch.float32, "vertices")
    _chk(faces, torch.int32, "faces")
    H, W = int(hw[0]), int(hw[1])
    if faces.shape[0] == 0:
        return torch.zeros((H, W), dtype=torch.float32, device=vertices.device)
    K = np.eye(3, dtype=np.float32)
    w2c = np.ascontiguousarray(P, dtype=np.float32).reshape(3, 4)
    zbuf = torch.full((H, W), -1, dtype=torch.int64, device=vertices.device)          # all ones = empty
    _lib.lib().surf_raster_first_hit(_p(vertices), _p(faces), faces.shape[0], _np_ptr(K), _np_ptr(w2c), H, W, H, W, _p(zbuf),
                                     _stream())
    depth = (zbuf >> 32).to(torch.int32).view(torch.float32)
    return torch.where(zbuf == -1, torch.zeros_like(depth), depth)


# ------------------------------------------------------------------------------------------------
# DTU Chamfer evaluation (dtu_eval.hip): mesh sampling, greedy thinning, capped nearest neighbour, all fp64
# ------------------------------------------------------------------------------------------------

THIN_AXIS_CELLS = 1 << 21        # cells per axis of a dtu_eval grid (63-bit keys)
NEAREST_MAX_CELLS = 1 << 26      # dense cell table of nearest_dist_capped


def _box(points):
    """Per-axis min and extent of a (n, 3) device tensor, on the host (one sync)."""
    lo, hi = points.amin(0).tolist(), points.amax(0).tolist()
    return lo, [b - a for a, b in zip(lo, hi)]


def _table_cell_dims(ext, n, floor_cell, max_cells, start_cell=None):
    """(cell, dims) of a dense cell table over a box of extents `ext` that holds n points.  The cell starts at start_cell or, by
    default, at about four cells per point by the volume of the padded box, at least floor_cell; it grows by 1.25 until the table
    has at most max_cells cells.  Pure host arithmetic."""
    cell = start_cell
    if cell is None:
        pad = max(ext) * 1e-3 or 1.0                  # flat or single-point clouds still get a box of some volume
        vol = (ext[0] + pad) * (ext[1] + pad) * (ext[2] + pad)
        cell = max((vol / (4.0 * n)) ** (1.0 / 3.0), floor_cell)
    while True:
        dims = [int(e // cell) + 1 for e in ext]
        if dims[0] * dims[1] * dims[2] <= max_cells:
            return cell, dims
        cell *= 1.25


def _cell_table(points, keys, ncell, tail=False):
    """(cstart (ncell + 1,) int32, the points in cell order, the sort order) of per-point cell keys: torch's sort, bincount and
    cumsum.  tail: keys may equal ncell (points that belong to no cell); those sort behind the table and are not counted."""
    skeys, order = torch.sort(keys)
    cstart = torch.zeros(ncell + 1, dtype=torch.int32, device=keys.device)
    counts = torch.bincount(skeys, minlength=ncell + 1)[:ncell] if tail else torch.bincount(skeys, minlength=ncell)
    cstart[1:] = torch.cumsum(counts, 0)
    return cstart, points[order].contiguous(), order


def mesh_sample_points(vertices, triangles, thresh):
    """dtu_eval.sample_mesh_points on the device: (nv + samples, 3) float64, the vertices followed by the lattice samples of
    every triangle of non-zero area, triangle by triangle.  vertices (nv, 3) float64, triangles (nt, 3) int64.  One host
    sync sizes the output (plus one that checks the triangle indices)."""
    _chk(vertices, torch.float64, "vertices")
    _chk(triangles, torch.int64, "triangles")
    nv, nt = vertices.shape[0], triangles.shape[0]
    if nt == 0:
        return vertices.clone()
    lo, hi = (int(v) for v in torch.stack([triangles.min(), triangles.max()]).tolist())
    if lo < 0 or hi >= nv:
        raise IndexError(f"triangles index vertices {lo}..{hi} of {nv}")
    L = _lib.lib()
    counts = torch.empty(nt, dtype=torch.int64, device=vertices.device)
    L.surf_dtu_sample_count(_p(vertices), _p(triangles), nt, float(thresh), _p(counts), _stream())
    ends = torch.cumsum(counts, 0)
    total = int(ends[-1])
    out = torch.empty(nv + total, 3, dtype=torch.float64, device=vertices.device)
    out[:nv] = vertices
    if total:
        L.surf_dtu_sample_write(_p(vertices), _p(triangles), nt, float(thresh), _p(ends - counts), _p(out[nv:]), _stream())
    return out


def thin_points(points, thresh, max_rounds=10000):
    """Greedy thinning of dtu_eval.downsample_points on already shuffled points (n, 3) float64: keep a point iff no earlier
    KEPT point lies within `thresh` ((dx*dx + dy*dy) + dz*dz <= thresh*thresh, scikit-learn's radius_neighbors test).
    Returns (keep (n,) bool, rounds): the parallel rounds it took, each ending in one host sync."""
    _chk(points, torch.float64, "points")
    n = points.shape[0]
    dev = points.device
    if n == 0:
        return torch.zeros(0, dtype=torch.bool, device=dev), 0
    if n > 2 ** 31 - 1:
        raise ValueError(f"thin_points: {n} points exceed int32 indexing")
    L = _lib.lib()
    lo, ext = _box(points)
    # cells a little wider than thresh (so that rounding in floor((p - lo) / cell) cannot push a neighbour two cells away),
    # wider still if an axis would need more than THIN_AXIS_CELLS
    cell = max(float(thresh) * (1 + 1e-6), max(ext) / (THIN_AXIS_CELLS - 2) * (1 + 1e-6))
    if not cell > 0:
        cell = 1.0
    A = THIN_AXIS_CELLS
    keys = torch.empty(n, dtype=torch.int64, device=dev)
    L.surf_dtu_cell_keys(_p(points), n, lo[0], lo[1], lo[2], cell, A, A, A, _p(keys), _stream())
    skeys, order = torch.sort(keys, stable=True)              # stable: a cell lists its points in shuffled order
    ucell, scell, counts = torch.unique_consecutive(skeys, return_inverse=True, return_counts=True)
    cstart = torch.zeros(ucell.shape[0] + 1, dtype=torch.int32, device=dev)
    cstart[1:] = torch.cumsum(counts, 0)
    spts = points[order].contiguous()
    sidx = order.to(torch.int32)
    scell = scell.to(torch.int32)
    state = torch.zeros(n, dtype=torch.int32, device=dev)
    undecided = torch.empty(1, dtype=torch.int32, device=dev)
    rounds = 0
    while True:
        L.surf_dtu_thin_round(_p(spts), _p(sidx), _p(scell), _p(ucell), _p(cstart), n, ucell.shape[0], float(thresh),
                              _p(state), _p(undecided), _stream())
        rounds += 1
        if int(undecided.item()) == 0:
            break
        if rounds >= max_rounds:
            raise RuntimeError(f"thin_points: {int(undecided.item())} of {n} points still undecided after {rounds} rounds")
    return state == 1, rounds


def nearest_dist_capped(queries, ref, max_dist):
    """Distance from every query (m, 3) float64 to its nearest reference point (r, 3) float64 where that is < max_dist, +inf
    elsewhere (scikit-learn's kneighbors(n_neighbors=1) distance, bit for bit).  Two host syncs (the reference box)."""
    _chk(queries, torch.float64, "queries")
    _chk(ref, torch.float64, "ref")
    m, r = queries.shape[0], ref.shape[0]
    dev = queries.device
    if not (max_dist > 0 and np.isfinite(max_dist)):
        raise ValueError(f"nearest_dist_capped: max_dist must be finite and > 0, got {max_dist}")
    if m == 0 or r == 0:
        return torch.full((m,), float("inf"), dtype=torch.float64, device=dev)
    if r > 2 ** 31 - 1:
        raise ValueError(f"nearest_dist_capped: {r} reference points exceed int32 indexing")
    L = _lib.lib()
    lo, ext = _box(ref)
    cell, dims = _table_cell_dims(ext, r, max(ext) / (THIN_AXIS_CELLS - 2), NEAREST_MAX_CELLS)
    keys = torch.empty(r, dtype=torch.int64, device=dev)
    L.surf_dtu_cell_keys(_p(ref), r, lo[0], lo[1], lo[2], cell, dims[0], dims[1], dims[2], _p(keys), _stream())
    cstart, sref, _ = _cell_table(ref, keys, dims[0] * dims[1] * dims[2])
    out = torch.empty(m, dtype=torch.float64, device=dev)
    L.surf_dtu_nearest(_p(queries), m, _p(sref), _p(cstart), lo[0], lo[1], lo[2], cell, dims[0], dims[1], dims[2],
                       float(max_dist), _p(out), _stream())
    return out


# ---- F-score evaluation (fscore.hip): transform, polygon crop, voxel mean, nearest with index, the ICP reductions, all fp64 ----

FSCORE_ICP_SLOTS = 1024          # SURF_FSCORE_ICP_SLOTS of include/surf_hip.h


def _chk_points(t, name):
    _chk(t, torch.float64, name)
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"{name}: expected (n, 3), got {tuple(t.shape)}")
    if t.shape[0] > 2 ** 31 - 1:
        raise ValueError(f"{name}: {t.shape[0]} points exceed int32 indexing")
    return t


def fscore_transform(points, T):
    """R p + t of (n, 3) float64 device points with the HOST 4x4 T, as ((R[k,0]*x + R[k,1]*y) + R[k,2]*z) + t[k]."""
    _chk_points(points, "points")
    T = np.ascontiguousarray(np.asarray(T, dtype=np.float64).reshape(4, 4))
    out = torch.empty_like(points)
    if points.shape[0] == 0:
        return out
    _lib.lib().surf_fscore_transform(_p(points), points.shape[0], _np_ptr(T), _p(out), _stream())
    return out


def fscore_crop(points, axis, axis_min, axis_max, polygon_uv):
    """keep (n,) bool: axis_min <= p[axis] <= axis_max and (u, v) = the two other coordinates inside polygon_uv (k, 2) float64
    (a device tensor) by the crossing-number rule of fscore.hip."""
    _chk_points(points, "points")
    _chk(polygon_uv, torch.float64, "polygon_uv")
    if polygon_uv.dim() != 2 or polygon_uv.shape[1] != 2 or polygon_uv.shape[0] < 3:
        raise ValueError(f"polygon_uv: expected (k >= 3, 2), got {tuple(polygon_uv.shape)}")
    if axis not in (0, 1, 2):
        raise ValueError(f"fscore_crop: axis must be 0, 1 or 2, got {axis}")
    n = points.shape[0]
    keep = torch.empty(n, dtype=torch.uint8, device=points.device)
    if n == 0:
        return keep.bool()
    _lib.lib().surf_fscore_crop(_p(points), n, int(axis), float(axis_min), float(axis_max), _p(polygon_uv), polygon_uv.shape[0],
                                _p(keep), _stream())
    return keep.bool()


def fscore_voxel_mean(points, voxel):
    """One point per occupied cell of the grid of `voxel` at min(points) - voxel / 2, in ascending (x << 42) | (y << 21) | z order:
    the members' sum in input order over their number ((m, 3) float64).  One host sync for the box, one for m."""
    _chk_points(points, "points")
    n = points.shape[0]
    dev = points.device
    if n == 0:
        return torch.empty(0, 3, dtype=torch.float64, device=dev)
    if not (voxel > 0 and np.isfinite(voxel)):
        raise ValueError(f"fscore_voxel_mean: voxel must be finite and > 0, got {voxel}")
    L = _lib.lib()
    lo = np.array(points.amin(0).tolist())
    hi = np.array(points.amax(0).tolist())
    keys = torch.empty(n, dtype=torch.int64, device=dev)
    L.surf_fscore_voxel_keys(_p(points), n, _np_ptr(lo), _np_ptr(hi), float(voxel), _p(keys), _stream())
    skeys, order = torch.sort(keys, stable=True)              # stable: a voxel lists its points in input order
    _, counts = torch.unique_consecutive(skeys, return_counts=True)
    m = counts.shape[0]
    seg = torch.zeros(m + 1, dtype=torch.int64, device=dev)
    seg[1:] = torch.cumsum(counts, 0)
    out = torch.empty(m, 3, dtype=torch.float64, device=dev)
    L.surf_fscore_voxel_mean(_p(points), n, _p(order), _p(seg), m, _p(out), _stream())
    return out


class NearestTable:
    """The dense cell table of nearest_dist_capped over one reference cloud, kept for several query sets (an ICP round asks the
    same target twenty times).  cells_per_point / cell / dims say how dense it came out."""

    def __init__(self, ref):
        _chk_points(ref, "ref")
        r = ref.shape[0]
        if r == 0:
            raise ValueError("NearestTable: empty reference")
        dev = ref.device
        lo, ext = _box(ref)
        cell, dims = _table_cell_dims(ext, r, max(ext) / (THIN_AXIS_CELLS - 2), NEAREST_MAX_CELLS)
        ncell = dims[0] * dims[1] * dims[2]
        keys = torch.empty(r, dtype=torch.int64, device=dev)
        _lib.lib().surf_dtu_cell_keys(_p(ref), r, lo[0], lo[1], lo[2], cell, dims[0], dims[1], dims[2], _p(keys), _stream())
        self.cstart, self.sref, order = _cell_table(ref, keys, ncell)
        self.sidx = order.to(torch.int32)
        self.lo, self.cell, self.dims, self.r = lo, cell, dims, r
        self.cells_per_point = ncell / r

    def query(self, queries, max_dist):
        _chk_points(queries, "queries")
        if not (max_dist > 0 and np.isfinite(max_dist)):
            raise ValueError(f"nearest_capped_index: max_dist must be finite and > 0, got {max_dist}")
        m = queries.shape[0]
        dist = torch.empty(m, dtype=torch.float64, device=queries.device)
        index = torch.empty(m, dtype=torch.int64, device=queries.device)
        if m:
            lo, d = self.lo, self.dims
            _lib.lib().surf_fscore_nearest(_p(queries), m, _p(self.sref), _p(self.sidx), _p(self.cstart), lo[0], lo[1], lo[2],
                                           self.cell, d[0], d[1], d[2], float(max_dist), _p(dist), _p(index), _stream())
        return dist, index


def nearest_capped_index(queries, ref, max_dist):
    """nearest_dist_capped plus WHICH reference point: (dist (m,) float64, +inf where >= max_dist; index (m,) int64 into ref, -1
    there).  Equal squared distances go to the smaller index.  ref may be a NearestTable."""
    _chk_points(queries, "queries")
    m = queries.shape[0]
    dev = queries.device
    if not (max_dist > 0 and np.isfinite(max_dist)):
        raise ValueError(f"nearest_capped_index: max_dist must be finite and > 0, got {max_dist}")
    if not isinstance(ref, NearestTable):
        _chk_points(ref, "ref")
        if m == 0 or ref.shape[0] == 0:
            return (torch.full((m,), float("inf"), dtype=torch.float64, device=dev),
                    torch.full((m,), -1, dtype=torch.int64, device=dev))
        ref = NearestTable(ref)
    return ref.query(queries, max_dist)


def _icp_args(source, target, index):
    _chk_points(source, "source")
    _chk_points(target, "target")
    _chk(index, torch.int64, "index")
    if index.shape != (source.shape[0],):
        raise ValueError(f"index: expected ({source.shape[0]},), got {tuple(index.shape)}")
    return torch.empty(FSCORE_ICP_SLOTS * 9, dtype=torch.float64, device=source.device)


def fscore_icp_sums(source, target, index, dist):
    """(8,) float64 device tensor [pairs, sum of source (3), sum of target (3), sum of dist^2] over the pairs (source[i],
    target[index[i]]), index[i] >= 0.  Fixed-slot partial sums added in slot order: the same bits on every run."""
    part = _icp_args(source, target, index)
    _chk(dist, torch.float64, "dist")
    if dist.shape != index.shape:
        raise ValueError(f"dist: expected {tuple(index.shape)}, got {tuple(dist.shape)}")
    out = torch.zeros(8, dtype=torch.float64, device=source.device)
    if source.shape[0] == 0 or target.shape[0] == 0:
        return out
    _lib.lib().surf_fscore_icp_sums(_p(source), _p(target), target.shape[0], _p(index), _p(dist), source.shape[0], _p(part), _p(out),
                                    _stream())
    return out


def fscore_icp_cov(source, target, index, centroid_source, centroid_target):
    """(3, 3) float64 device tensor H[r][c] = sum (source[r] - cs[r]) * (target[index][c] - ct[c]) over the same pairs, reduced
    like fscore_icp_sums; the centroids are host triples."""
    part = _icp_args(source, target, index)
    out = torch.zeros(9, dtype=torch.float64, device=source.device)
    if source.shape[0] == 0 or target.shape[0] == 0:
        return out.reshape(3, 3)
    c = np.ascontiguousarray(np.concatenate([np.asarray(centroid_source, dtype=np.float64).reshape(3),
                                             np.asarray(centroid_target, dtype=np.float64).reshape(3)]))
    _lib.lib().surf_fscore_icp_cov(_p(source), _p(target), target.shape[0], _p(index), source.shape[0], _np_ptr(c), _p(part), _p(out),
                                   _stream())
    return out.reshape(3, 3)


# ------------------------------------------------------------------------------------------------
# mesh cleaning (mesh_clean.hip): dilation, visual hull, visible faces, face components, compaction
# ------------------------------------------------------------------------------------------------


def _camera_rows(intrs, c2ws, dev):
    """(nv, 21) fp32 device rows [K row-major | inverse(c2w)[:3, :4] row-major], computed on the host as raster_first_hit
    computes them."""
    rows = [torch.cat([K.detach().to("cpu", torch.float32)[:3, :3].reshape(-1),
                       torch.inverse(c2w.detach().to("cpu", torch.float32))[:3, :4].reshape(-1)])
            for K, c2w in zip(intrs, c2ws)]
    return torch.stack(rows).contiguous().to(dev)


def clean_dilate(masks, radius):
    """clean_mesh.dilate_disk of every (h, w) slice of masks (nv, h, w) uint8 / bool on the device; returns bool."""
    m = masks.view(torch.uint8) if masks.dtype == torch.bool else masks
    _chk(m, torch.uint8, "masks")
    assert m.dim() == 3
    out = torch.empty_like(m)
    if m.numel():
        nv, h, w = m.shape
        _lib.lib().surf_clean_dilate(_p(m), nv, h, w, int(radius), _p(out), _stream())
    return out.view(torch.bool)


def clean_hull_count(vertices, masks, intrs, c2ws):
    """Per-vertex number of views that see the vertex (clean_mesh.clean_mesh_by_mask's n_seen), int32.  vertices (n, 3) fp32,
    masks (nv, h, w) uint8 / bool on the device, intrs / c2ws host or device (nv, 4, 4)."""
    _chk(vertices, torch.float32, "vertices")
    m = masks.view(torch.uint8) if masks.dtype == torch.bool else masks
    _chk(m, torch.uint8, "masks")
    nv, h, w = m.shape
    n = vertices.shape[0]
    n_seen = torch.zeros(n, dtype=torch.int32, device=vertices.device)
    if n == 0 or nv == 0:
        return n_seen
    cams = _camera_rows(intrs, c2ws, vertices.device)
    _lib.lib().surf_clean_hull_count(_p(vertices), n, _p(m), _p(cams), nv, h, w, _p(n_seen), _stream())
    return n_seen


def clean_face_keep(n_seen, faces, min_nb_visible):
    """keep (F,) bool: each vertex of the face has n_seen > min_nb_visible."""
    _chk(n_seen, torch.int32, "n_seen")
    _chk(faces, torch.int32, "faces")
    keep = torch.empty(faces.shape[0], dtype=torch.uint8, device=faces.device)
    if faces.shape[0]:
        _lib.lib().surf_clean_face_keep(_p(n_seen), _p(faces), faces.shape[0], int(min_nb_visible), _p(keep), _stream())
    return keep.view(torch.bool)


def clean_visible_faces(vertices, faces, masks, intrs, c2ws, upscale):
    """clean_mesh.visible_faces without the up-scaled mask, the id image and the gather: per view, the z-buffer of
    surf_raster_first_hit and one marking pass.  masks (nv, h, w) uint8 / bool on the device; returns (F,) bool."""
    _chk(vertices, torch.float32, "vertices")
    _chk(faces, torch.int32, "faces")
    m = masks.view(torch.uint8) if masks.dtype == torch.bool else masks
    _chk(m, torch.uint8, "masks")
    if int(upscale) != upscale or upscale < 1:
        raise ValueError("the device cleaner takes an integer upscale >= 1")
    upscale = int(upscale)
    nv, h, w = m.shape
    nf = faces.shape[0]
    seen = torch.zeros(nf, dtype=torch.uint8, device=faces.device)
    if nf == 0 or nv == 0:
        return seen.view(torch.bool)
    Hup, Wup = h * upscale, w * upscale
    zbuf = torch.empty(Hup, Wup, dtype=torch.int64, device=faces.device)
    L = _lib.lib()
    for i in range(nv):                                   # launches only: nothing in this loop waits for the device
        K = np.ascontiguousarray(intrs[i].detach().to("cpu", torch.float32)[:3, :3].contiguous().numpy())
        w2c = np.ascontiguousarray(torch.inverse(c2ws[i].detach().to("cpu", torch.float32))[:3, :4].contiguous().numpy())
        zbuf.fill_(-1)
        L.surf_raster_first_hit(_p(vertices), _p(faces), nf, _np_ptr(K), _np_ptr(w2c), h, w, Hup, Wup, _p(zbuf), _stream())
        L.surf_clean_mark_visible(_p(zbuf), Hup, Wup, _p(m[i]), h, w, upscale, nf, _p(seen), _stream())
    return seen.view(torch.bool)


def clean_components(faces, min_len, return_labels=False):
    """clean_mesh.face_components on the device: keep (F,) bool of the faces that share an edge with some face and whose
    edge-connected component has at least min_len faces.  faces (F, 3) int32.  With return_labels also (root, size): the
    smallest face id of every face's component and, at the roots, the component's face count."""
    _chk(faces, torch.int32, "faces")
    nf, dev = faces.shape[0], faces.device
    if nf == 0:
        e = torch.zeros(0, dtype=torch.bool, device=dev)
        return (e, torch.zeros(0, dtype=torch.int32, device=dev), torch.zeros(0, dtype=torch.int32, device=dev)) if return_labels else e
    L = _lib.lib()
    slots = L.surf_clean_components_slots(nf)
    if slots < 0:       # an int64_t size query reports its SURF_E_* through the value: no errcheck is bound, so checked here
        _lib.check(int(slots), "surf_clean_components_slots")
    try:
        keys = torch.empty(slots, dtype=torch.int64, device=dev)
        owner = torch.empty(slots, dtype=torch.int32, device=dev)
        shared = torch.empty(slots, dtype=torch.uint8, device=dev)
        edge_slot = torch.empty(3 * nf, dtype=torch.int32, device=dev)
        parent = torch.empty(nf, dtype=torch.int32, device=dev)
        size = torch.empty(nf, dtype=torch.int32, device=dev)
        has_nb = torch.empty(nf, dtype=torch.uint8, device=dev)
        keep = torch.empty(nf, dtype=torch.uint8, device=dev)
    except torch.cuda.OutOfMemoryError:     # no entry point was called: the limit error is raised in the library's words
        _lib.check(-2, f"surf_clean_components: the edge table of {nf} faces does not fit the device")
    L.surf_clean_components(_p(faces), nf, int(min(max(int(min_len), -1), 1 << 62)), _p(keys), _p(owner), _p(shared), slots,
                            _p(edge_slot), _p(parent), _p(has_nb), _p(size), _p(keep), _stream())
    keep = keep.view(torch.bool)
    return (keep, parent, size) if return_labels else keep


def clean_update_faces(vertices, faces, keep, compact_vertices=True):
    """clean_mesh.update_faces on the device: the kept faces in their order and, with compact_vertices, the vertices they use
    in their order with the faces renumbered.  vertices (V, 3) of any 4- or 8-byte dtype (returned in that dtype), faces (F, 3)
    int32, keep (F,) bool / uint8.  One host read (the two counts)."""
    _chk(faces, torch.int32, "faces")
    if not torch.is_tensor(vertices) or not vertices.is_contiguous() or vertices.element_size() not in (4, 8):
        raise TypeError("vertices: expected a contiguous tensor of a 4- or 8-byte dtype")
    k = keep.view(torch.uint8) if keep.dtype == torch.bool else keep
    _chk(k, torch.uint8, "keep")
    nf, nv, dev = faces.shape[0], vertices.shape[0], faces.device
    if nf == 0 or nv == 0:
        return (vertices[:0] if compact_vertices else vertices), faces[:0]
    L = _lib.lib()
    fscan = torch.cumsum(k, 0, dtype=torch.int64)
    if compact_vertices:
        used = torch.zeros(nv, dtype=torch.uint8, device=dev)
        L.surf_clean_mark_used(_p(faces), _p(k), nf, nv, _p(used), _stream())
        vscan = torch.cumsum(used, 0, dtype=torch.int64)
        n_f, n_v = (int(v) for v in torch.stack([fscan[-1], vscan[-1]]).tolist())
    else:
        used = vscan = None
        n_f, n_v = int(fscan[-1].item()), nv
    out_f = torch.empty(n_f, 3, dtype=torch.int32, device=dev)
    if n_f:
        L.surf_clean_compact_faces(_p(faces), _p(k), _p(fscan), _p(vscan), nf, nv, _p(out_f), _stream())
    if not compact_vertices:
        return vertices, out_f
    out_v = torch.empty(n_v, 3, dtype=vertices.dtype, device=dev)
    if n_v:
        L.surf_clean_compact_rows(_p(vertices), vertices.element_size(), _p(used), _p(vscan), nv, _p(out_v), _stream())
    return out_v, out_f


# ------------------------------------------------------------------------------------------------
# mesh simplification (mesh_simplify.hip): vertex clustering with quadric placement; the rule is in include/surf_hip.h
# ------------------------------------------------------------------------------------------------

SIMPLIFY_HOST_READS = 2          # simplify_mesh waits for the device twice: see its docstring


def simplify_mesh(vertices, faces, cell, normals=None, colors=None, stages=None):
    """The surf_simplify_* rule on device tensors: vertices (n, 3) fp32, faces (m, 3) int32, optional normals (n, 3) fp32 and
    colors (n, 3) uint8 -> (vertices (k, 3) fp32, faces (j, 3) int32, normals or None, colors or None, vertex_map (n,) int32).
    The sorts, scans and searches between the kernels are torch's.  Exactly SIMPLIFY_HOST_READS reads of the device, each one
    small copy: (1) [number of cells, limit flag, smallest and largest face index], (2) [kept faces, used cells]; an empty mesh
    reads nothing.  A vertex outside the rule's lattice, or a face index outside the vertex list, raises ValueError after (1).
    stages: a list that receives (name, start event, end event) per stage (scripts/time_simplify.py)."""
    _chk(vertices, torch.float32, "vertices")
    _chk(faces, torch.int32, "faces")
    if vertices.dim() != 2 or vertices.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"simplify_mesh: expected (n, 3) vertices and (m, 3) faces, got {tuple(vertices.shape)}, {tuple(faces.shape)}")
    n, m, dev = vertices.shape[0], faces.shape[0], vertices.device
    if max(n, m) > (2 ** 31 - 1) // 3:
        _lib.check(-2, f"simplify_mesh: {n} vertices / {m} faces")
    for t, dtype, name in ((normals, torch.float32, "normals"), (colors, torch.uint8, "colors")):
        if t is not None:
            _chk(t, dtype, name)
            if tuple(t.shape) != (n, 3):
                raise ValueError(f"simplify_mesh: {name} {tuple(t.shape)} for {n} vertices")
    cell = float(cell)
    if not (cell > 0 and 0 < cell * cell < float("inf")):
        raise ValueError(f"simplify_mesh: cell must be finite and > 0, got {cell}")

    def empty():
        return (vertices.new_empty(0, 3), faces.new_empty(0, 3), None if normals is None else normals.new_empty(0, 3),
                None if colors is None else colors.new_empty(0, 3), torch.full((n,), -1, dtype=torch.int32, device=dev))

    if n == 0 or m == 0:
        return empty()

    def stage(name):
        if stages is not None:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            if stages:
                stages[-1] = stages[-1][:2] + (ev,)
            if name is not None:
                stages.append((name, ev, None))

    L, s = _lib.lib(), _stream()
    stage("keys+sort")
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    keys = torch.empty(n, dtype=torch.int64, device=dev)
    L.surf_simplify_keys(_p(vertices), n, cell, _p(keys), _p(flag), s)
    skeys, vorder = torch.sort(keys, stable=True)                      # stable: a cell lists its vertices in index order
    head = torch.ones(n, dtype=torch.bool, device=dev)
    head[1:] = skeys[1:] != skeys[:-1]
    rank = torch.cumsum(head, 0, dtype=torch.int64) - 1
    f_lo, f_hi = torch.aminmax(faces)
    n_cells, bad, lo, hi = torch.stack([rank[-1] + 1, flag[0].long(), f_lo.long(), f_hi.long()]).tolist()       # host read 1
    if bad:
        raise ValueError(f"simplify_mesh: a vertex is not finite or lies outside the 2^21 cells of {cell} per axis "
                         "(surf_simplify_keys: exceeds a SURF_MAX_* limit)")
    if lo < 0 or hi >= n:
        raise ValueError(f"face indices span [{lo}, {hi}], the mesh has {n} vertices")
    stage("faces")
    vcell = torch.empty(n, dtype=torch.int32, device=dev)
    vstart = torch.empty(n_cells + 1, dtype=torch.int64, device=dev)
    L.surf_simplify_segments(_p(skeys), _p(vorder), _p(rank), n, n_cells, _p(vcell), _p(vstart), s)
    fcell = torch.empty(m, 3, dtype=torch.int32, device=dev)
    L.surf_simplify_face_cells(_p(faces), m, _p(vcell), n, _p(fcell), _p(flag), s)
    slots = 1024
    while slots < 2 * m:
        slots <<= 1
    owner = torch.empty(slots, dtype=torch.int32, device=dev)
    face_slot = torch.empty(m, dtype=torch.int32, device=dev)
    keep = torch.empty(m, dtype=torch.uint8, device=dev)
    L.surf_simplify_faces(_p(fcell), m, _p(owner), slots, _p(face_slot), _p(keep), s)
    used = torch.zeros(n_cells, dtype=torch.uint8, device=dev)
    L.surf_simplify_mark_used(_p(fcell), _p(keep), m, n_cells, _p(used), s)
    fscan = torch.cumsum(keep, 0, dtype=torch.int64)
    cscan = torch.cumsum(used, 0, dtype=torch.int64)
    n_f, n_v = torch.stack([fscan[-1], cscan[-1]]).tolist()                                                 # host read 2
    if n_f == 0:
        stage(None)
        return empty()
    stage("corner sort")
    scell, corder = torch.sort(fcell.reshape(-1), stable=True)         # stable: a cell lists its corners in (face, corner) order
    cstart = torch.searchsorted(scell, torch.arange(n_cells + 1, dtype=torch.int32, device=dev))     # int64; no host read
    stage("cells")
    out_v = torch.empty(n_v, 3, dtype=torch.float32, device=dev)
    out_n = None if normals is None else torch.empty(n_v, 3, dtype=torch.float32, device=dev)
    out_c = None if colors is None else torch.empty(n_v, 3, dtype=torch.uint8, device=dev)
    L.surf_simplify_cells(_p(vertices), _p(normals), _p(colors), n, _p(faces), m, cell, _p(skeys), _p(vorder), _p(vstart),
                          _p(corder), _p(cstart), n_cells, _p(used), _p(cscan), _p(out_v), _p(out_n), _p(out_c), s)
    stage("compact")
    out_f = torch.empty(n_f, 3, dtype=torch.int32, device=dev)
    vmap = torch.empty(n, dtype=torch.int32, device=dev)
    L.surf_simplify_compact(_p(fcell), _p(keep), _p(fscan), m, _p(vcell), n, _p(used), _p(cscan), n_cells, _p(out_f), _p(vmap), s)
    stage(None)
    return out_v, out_f, out_n, out_c, vmap


# ------------------------------------------------------------------------------------------------
# mesh smoothing (mesh_smooth.hip): Laplacian / Taubin steps with uniform weights; the rule is in include/surf_hip.h
# ------------------------------------------------------------------------------------------------

SMOOTH_HOST_READS = 2            # smooth_mesh waits for the device twice: see its docstring
SMOOTH_MAX_ITEMS = (2 ** 31 - 1) // 6
_SMOOTH_NO_KEY = 2 ** 63 - 1


def smooth_adjacency(faces, n, also=()):
    """Rule 1 of the surf_smooth_* group on a device tensor faces (m, 3) int32 of a mesh with n vertices, m, n >= 1:
    (row_start (n + 1) int32, neighbours (nnz) int32, boundary (n) uint8, values of `also`).  neighbours[row_start[i] :
    row_start[i + 1]] is N(i) ascending.  One read of the device: [nnz, smallest and largest face index] and the 0-dim tensors of
    `also`, whose values come back as Python numbers; a face index outside [0, n) raises ValueError after it."""
    _chk(faces, torch.int32, "faces")
    m, dev = faces.shape[0], faces.device
    if max(n, m) > SMOOTH_MAX_ITEMS:
        _lib.check(-2, f"smooth_mesh: {n} vertices / {m} faces")
    L, s = _lib.lib(), _stream()
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    keys = torch.empty(6 * m, dtype=torch.int64, device=dev)
    L.surf_smooth_edge_keys(_p(faces), m, n, _p(keys), _p(flag), s)
    skeys = torch.sort(keys)[0]
    del keys
    head = torch.ones(6 * m, dtype=torch.bool, device=dev)
    head[1:] = skeys[1:] != skeys[:-1]
    hscan = torch.cumsum(head, 0, dtype=torch.int64)
    # the first entry of every row: the runs in front of the first key >= (v << 32); every key below NO_KEY is below (n << 32)
    pos = torch.searchsorted(skeys, torch.arange(n + 1, dtype=torch.int64, device=dev) << 32)
    starts = torch.where(pos > 0, hscan[(pos - 1).clamp_(min=0)], torch.zeros_like(pos))
    f_lo, f_hi = torch.aminmax(faces)
    read = torch.stack([starts[n].double(), f_lo.double(), f_hi.double()] + [t.double() for t in also]).tolist()      # host read
    nnz, lo, hi = (int(x) for x in read[:3])
    if lo < 0 or hi >= n:
        raise ValueError(f"face indices span [{lo}, {hi}], the mesh has {n} vertices")
    neighbours = torch.empty(nnz, dtype=torch.int32, device=dev)
    boundary = torch.zeros(n, dtype=torch.uint8, device=dev)
    L.surf_smooth_adjacency(_p(skeys), _p(hscan), m, n, nnz, _p(neighbours), _p(boundary), s)
    return starts.to(torch.int32), neighbours, boundary, read[3:]


def smooth_normals(vertices, faces, given=None):
    """Rule 5 of the surf_smooth_* group on device tensors: (n, 3) fp32 vertex normals of vertices (n, 3) fp32 and faces (m, 3)
    int32, kept on the side of `given` (n, 3) fp32 when that is not None.  No read of the device; the face indices must be valid."""
    _chk(vertices, torch.float32, "vertices")
    _chk(faces, torch.int32, "faces")
    n, m, dev = vertices.shape[0], faces.shape[0], vertices.device
    if max(n, m) > SMOOTH_MAX_ITEMS:
        _lib.check(-2, f"smooth_normals: {n} vertices / {m} faces")
    if given is not None:
        _chk(given, torch.float32, "normals")
        if tuple(given.shape) != (n, 3):
            raise ValueError(f"smooth_mesh: normals {tuple(given.shape)} for {n} vertices")
    out = torch.empty(n, 3, dtype=torch.float32, device=dev)
    sorted_v, corder = torch.sort(faces.reshape(-1), stable=True)      # stable: a vertex lists its corners in (face, corner) order
    cstart = torch.searchsorted(sorted_v, torch.arange(n + 1, dtype=torch.int32, device=dev))
    scratch = torch.empty(m, 3, dtype=torch.float64, device=dev)
    _lib.lib().surf_smooth_normals(_p(vertices), n, _p(faces), m, _p(corder), _p(cstart), _p(given), _p(scratch), _p(out), _stream())
    return out


def smooth_mesh(vertices, faces, iterations=10, lam=0.5, mu=-0.53, pin_boundary=True, max_move=None, normals=None, stages=None):
    """The surf_smooth_* rule on device tensors: vertices (n, 3) fp32, faces (m, 3) int32, normals None, True or (n, 3) fp32 ->
    (vertices (n, 3) fp32, normals (n, 3) fp32 or None, info); the arguments and info are surf_amd.mesh_smooth.smooth_mesh's.
    The sorts, scans and searches between the kernels are torch's.  Exactly SMOOTH_HOST_READS reads of the device, each one small
    copy: (1) [number of neighbour entries, smallest and largest face index, all vertices finite] before any step, (2) [boundary
    vertices, isolated vertices, largest and summed squared movement, capped vertices] for info; an empty mesh reads nothing.  A
    face index outside the vertex list or a vertex that is not finite raises ValueError after (1), before any step.
    stages: a list that receives (name, start event, end event) per stage (scripts/time_mesh_smooth.py)."""
    from .mesh_smooth import check_args, schedule
    _chk(vertices, torch.float32, "vertices")
    _chk(faces, torch.int32, "faces")
    if vertices.dim() != 2 or vertices.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"smooth_mesh: expected (n, 3) vertices and (m, 3) faces, got {tuple(vertices.shape)}, {tuple(faces.shape)}")
    iterations, lam, mu, pin_boundary, max_move = check_args(iterations, lam, mu, pin_boundary, max_move)
    n, m, dev = vertices.shape[0], faces.shape[0], vertices.device
    if max(n, m) > SMOOTH_MAX_ITEMS:
        _lib.check(-2, f"smooth_mesh: {n} vertices / {m} faces")
    given = None if normals is None or normals is True else normals
    if given is not None:
        _chk(given, torch.float32, "normals")
        if tuple(given.shape) != (n, 3):
            raise ValueError(f"smooth_mesh: normals {tuple(given.shape)} for {n} vertices")
    if n == 0 or m == 0:
        nrm = given if given is not None else (torch.zeros(n, 3, dtype=torch.float32, device=dev) if normals is True else None)
        return vertices, nrm, {"vertices": n, "boundary_vertices": 0, "isolated_vertices": n, "moved_max": 0.0, "moved_rms": 0.0,
                               "capped": 0}

    def stage(name):
        if stages is not None:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            if stages:
                stages[-1] = stages[-1][:2] + (ev,)
            if name is not None:
                stages.append((name, ev, None))

    L, s = _lib.lib(), _stream()
    stage("adjacency")
    row_start, neighbours, boundary, (finite,) = smooth_adjacency(faces, n, also=(torch.isfinite(vertices).all(),))   # host read 1
    if not finite:
        i = int(torch.nonzero(~torch.isfinite(vertices).all(dim=1))[0, 0])
        raise ValueError(f"smooth_mesh: vertex {i} is not finite: {vertices[i].tolist()}")
    nnz = neighbours.shape[0]
    stage("steps")
    a = torch.zeros(n, 4, dtype=torch.float32, device=dev)             # 16-byte rows: a neighbour is one load
    a[:, :3] = vertices
    b = torch.empty_like(a)
    for factor in schedule(iterations, lam, mu):
        L.surf_smooth_step(_p(a), _p(b), n, _p(row_start), _p(neighbours), nnz, _p(boundary), int(pin_boundary), factor, s)
        a, b = b, a
    stage("cap")
    out = torch.empty(n, 3, dtype=torch.float32, device=dev)
    moved2 = torch.empty(n, dtype=torch.float64, device=dev)
    capped = torch.empty(n, dtype=torch.uint8, device=dev)
    L.surf_smooth_cap(_p(a), _p(vertices), n, 0.0 if max_move is None else max_move, _p(out), _p(moved2), _p(capped), s)
    total = moved2
    while total.shape[0] > 1:                                          # rule 4's 256-ary sequential tree
        runs = torch.empty((total.shape[0] + 255) // 256, dtype=torch.float64, device=dev)
        L.surf_smooth_sum256(_p(total), total.shape[0], _p(runs), s)
        total = runs
    nrm = None
    if normals is not None:
        stage("normals")
        nrm = smooth_normals(out, faces, given)
    stage(None)
    isolated = (row_start[1:] == row_start[:-1]).sum()
    nb, ni, qmax, qsum, nc = torch.stack([boundary.sum().double(), isolated.double(), moved2.max(), total[0],
                                          capped.sum().double()]).tolist()                                   # host read 2
    info = {"vertices": n, "boundary_vertices": int(nb), "isolated_vertices": int(ni), "moved_max": float(np.sqrt(qmax)),
            "moved_rms": float(np.sqrt(qsum / float(n))), "capped": int(nc)}
    return out, nrm, info


# ------------------------------------------------------------------------------------------------
# mesh denoising (mesh_denoise.hip): two-stage bilateral normal filtering; the rule is in include/surf_hip.h
# ------------------------------------------------------------------------------------------------

DENOISE_HOST_READS = 3           # denoise_mesh waits for the device three times: see its docstring


def _sum256(values):
    """The 256-ary sequential tree of smoothing rule 4 over a device tensor of fp64 values (at least one): a 1-element tensor."""
    L, s, total = _lib.lib(), _stream(), values
    while total.shape[0] > 1:
        runs = torch.empty((total.shape[0] + 255) // 256, dtype=torch.float64, device=values.device)
        L.surf_smooth_sum256(_p(total), total.shape[0], _p(runs), s)
        total = runs
    return total


def denoise_corners(faces, n):
    """(corner_order (3 m) int64, corner_start (n + 1) int64) of device faces (m, 3) int32, as surf_smooth_normals takes them."""
    sorted_v, corder = torch.sort(faces.reshape(-1), stable=True)      # stable: a vertex lists its corners in (face, corner) order
    cstart = torch.searchsorted(sorted_v, torch.arange(n + 1, dtype=torch.int32, device=faces.device))
    return corder, cstart


def denoise_neighbours(faces, n, corners=None, also=()):
    """Rule 3 of the surf_denoise_* group on a device tensor faces (m, 3) int32 with valid indices, m, n >= 1: (face_row_start
    (m + 1) int32, face_neighbours (total) int32, values of `also`).  One read of the device: the total and the 0-dim tensors of
    `also`; a total above 2^31 - 1 raises SurfHipError after it, before the list is allocated."""
    from .mesh_denoise import MAX_NEIGHBOURS
    _chk(faces, torch.int32, "faces")
    m, dev = faces.shape[0], faces.device
    if max(n, m) > SMOOTH_MAX_ITEMS:
        _lib.check(-2, f"denoise_mesh: {n} vertices / {m} faces")
    L, s = _lib.lib(), _stream()
    corder, cstart = denoise_corners(faces, n) if corners is None else corners
    counts = torch.empty(m, dtype=torch.int64, device=dev)
    L.surf_denoise_neighbour_count(_p(faces), m, n, _p(corder), _p(cstart), _p(counts), s)
    rows = torch.zeros(m + 1, dtype=torch.int64, device=dev)
    torch.cumsum(counts, 0, out=rows[1:])
    read = torch.stack([rows[m].double()] + [t.double() for t in also]).tolist()                              # host read
    total = int(read[0])
    if total > MAX_NEIGHBOURS:
        _lib.check(-2, f"denoise_mesh: {total} face neighbours")
    rows = rows.to(torch.int32)
    nbr = torch.empty(total, dtype=torch.int32, device=dev)
    L.surf_denoise_neighbour_emit(_p(faces), m, n, _p(corder), _p(cstart), _p(rows), total, _p(nbr), s)
    return rows, nbr, read[1:]


def denoise_mesh(vertices, faces, normal_iterations=10, vertex_iterations=10, sigma_r=0.35, sigma_s=None, pin_boundary=True,
                 max_move=None, normals=None, stages=None, keep=None):
    """The surf_denoise_* rule on device tensors: vertices (n, 3) fp32, faces (m, 3) int32, normals None, True or (n, 3) fp32 ->
    (vertices (n, 3) fp32, normals (n, 3) fp32 or None, info); the arguments and info are surf_amd.mesh_denoise.denoise_mesh's.
    The sorts, scans and searches between the kernels are torch's.  At most DENOISE_HOST_READS reads of the device, each one small
    copy: (1) smooth_adjacency's [neighbour entries, smallest and largest face index, all vertices finite], (2) [face neighbour
    total, summed side lengths] when there is a normal iteration or sigma_s is absent, (3) [boundary vertices, degenerate faces,
    largest and summed squared movement, capped vertices] for info; an empty mesh reads nothing.  A face index outside the vertex
    list or a vertex that is not finite raises ValueError after (1), a mean side length that is not > 0 after (2).
    stages: a list that receives (name, start event, end event) per stage (scripts/time_mesh_denoise.py).  keep: a dict that
    receives the tensors face_row_start, face_neighbours (when there is a normal iteration) and records (m, 8) after the normal
    stage."""
    from .mesh_denoise import check_args, inverse_supports, mean_side
    _chk(vertices, torch.float32, "vertices")
    _chk(faces, torch.int32, "faces")
    if vertices.dim() != 2 or vertices.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"denoise_mesh: expected (n, 3) vertices and (m, 3) faces, got {tuple(vertices.shape)}, {tuple(faces.shape)}")
    normal_iterations, vertex_iterations, sigma_r, sigma_s, pin_boundary, max_move = check_args(
        normal_iterations, vertex_iterations, sigma_r, sigma_s, pin_boundary, max_move)
    n, m, dev = vertices.shape[0], faces.shape[0], vertices.device
    if max(n, m) > SMOOTH_MAX_ITEMS:
        _lib.check(-2, f"denoise_mesh: {n} vertices / {m} faces")
    given = None if normals is None or normals is True else normals
    if given is not None:
        _chk(given, torch.float32, "normals")
        if tuple(given.shape) != (n, 3):
            raise ValueError(f"denoise_mesh: normals {tuple(given.shape)} for {n} vertices")
    if n == 0 or m == 0:
        nrm = given if given is not None else (torch.zeros(n, 3, dtype=torch.float32, device=dev) if normals is True else None)
        return vertices, nrm, {"vertices": n, "faces": m, "degenerate_faces": 0, "boundary_vertices": 0, "sigma_s": sigma_s,
                               "sigma_r": sigma_r, "moved_max": 0.0, "moved_rms": 0.0, "capped": 0}

    def stage(name):
        if stages is not None:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            if stages:
                stages[-1] = stages[-1][:2] + (ev,)
            if name is not None:
                stages.append((name, ev, None))

    L, s = _lib.lib(), _stream()
    stage("adjacency")
    _, _, boundary, (finite,) = smooth_adjacency(faces, n, also=(torch.isfinite(vertices).all(),))           # host read 1
    if not finite:
        i = int(torch.nonzero(~torch.isfinite(vertices).all(dim=1))[0, 0])
        raise ValueError(f"denoise_mesh: vertex {i} is not finite: {vertices[i].tolist()}")
    stage("records")
    corners = denoise_corners(faces, n)
    records = torch.empty(m, 8, dtype=torch.float32, device=dev)
    sides = torch.empty(m, 3, dtype=torch.float64, device=dev) if sigma_s is None else None
    L.surf_denoise_face_records(_p(vertices), n, _p(faces), m, _p(records), _p(sides), s)
    also = () if sides is None else (_sum256(sides.reshape(-1))[0],)
    rows = nbr = None
    if normal_iterations:
        stage("neighbours")
        rows, nbr, read = denoise_neighbours(faces, n, corners, also)                                         # host read 2
    else:
        read = torch.stack(list(also)).tolist() if also else []                                               # host read 2
    if sigma_s is None:
        sigma_s = mean_side(read[0], m)
    inv_s, inv_r = inverse_supports(sigma_s, sigma_r)
    if normal_iterations:
        stage("normal_steps")
        other = records.clone()                                        # areas and centroids in both buffers
        for _ in range(normal_iterations):
            L.surf_denoise_normal_step(_p(records), _p(other), m, _p(rows), _p(nbr), nbr.shape[0], inv_s, inv_r, s)
            records, other = other, records
        del other
    if keep is not None:
        keep.update(records=records)
        if rows is not None:
            keep.update(face_row_start=rows, face_neighbours=nbr)
    stage("vertex_steps")
    a = torch.zeros(n, 4, dtype=torch.float32, device=dev)             # 16-byte rows: a corner's position is one load
    a[:, :3] = vertices
    if vertex_iterations:
        b = torch.empty_like(a)
        for _ in range(vertex_iterations):
            L.surf_denoise_vertex_step(_p(a), _p(b), n, _p(faces), m, _p(records), _p(corners[0]), _p(corners[1]), _p(boundary),
                                       int(pin_boundary), s)
            a, b = b, a
    stage("cap")
    out = torch.empty(n, 3, dtype=torch.float32, device=dev)
    moved2 = torch.empty(n, dtype=torch.float64, device=dev)
    capped = torch.empty(n, dtype=torch.uint8, device=dev)
    L.surf_smooth_cap(_p(a), _p(vertices), n, 0.0 if max_move is None else max_move, _p(out), _p(moved2), _p(capped), s)
    total = _sum256(moved2)
    nrm = None
    if normals is not None:
        stage("normals")
        nrm = smooth_normals(out, faces, given)
    stage(None)
    degenerate = (records[:, :3] == 0).all(dim=1).sum()
    nb, nd, qmax, qsum, nc = torch.stack([boundary.sum().double(), degenerate.double(), moved2.max(), total[0],
                                          capped.sum().double()]).tolist()                                   # host read 3
    info = {"vertices": n, "faces": m, "degenerate_faces": int(nd), "boundary_vertices": int(nb), "sigma_s": sigma_s,
            "sigma_r": sigma_r, "moved_max": float(np.sqrt(qmax)), "moved_rms": float(np.sqrt(qsum / float(n))), "capped": int(nc)}
    return out, nrm, info


# ------------------------------------------------------------------------------------------------
# mesh deviation (mesh_distance.hip): exact point-to-triangle distances; the rule is in include/surf_hip.h
# ------------------------------------------------------------------------------------------------

def texture_pack_view(image, depth):
    """surf_texture_pack_view: image (H, W, 3) and depth (H, W) fp32 -> the (H, W, 4) records (r, g, b, D) surf_texture_bake taps."""
    _chk(image, torch.float32, "image")
    _chk(depth, torch.float32, "depth")
    H, W = (int(s) for s in depth.shape)
    if depth.dim() != 2 or tuple(image.shape) != (H, W, 3):
        raise ValueError(f"texture_pack_view: image (H, W, 3) and depth (H, W), got {tuple(image.shape)} and {tuple(depth.shape)}")
    record = torch.empty((H, W, 4), dtype=torch.float32, device=image.device)
    _lib.lib().surf_texture_pack_view(_p(image), _p(depth), H, W, _p(record), _stream())
    return record


def bake_texture(vertices, faces, views, T, cols, rows, depth_tol, min_cos=0.2, power=4, two_sided=False, z_min=0.0, fill=0.5,
                 vertex_colors=None, count=False, chunk=None, stages=None):
    """The device path of mesh_texture.bake_texture (the rule: include/surf_hip.h above surf_texture_*): vertices (n, 3) fp32,
    faces (m >= 1, 3) int32 and vertex_colors (n, 3) uint8 or None on the device; views: (P (12,) fp32 and centre (3,) fp32 on the
    host, image (H, W, 3) and mesh depth (H, W) fp32 on the device) in order; (cols, rows): mesh_texture.atlas_layout's.  The
    views go `chunk` (<= FUSE_MAX_VIEWS) to a launch; their packed records live only for their launch, and the accumulators stay
    in memory between launches.  Returns (atlas (Ha, Wa, 3) uint8, sums (Ha, Wa, 4) fp32, count (Ha, Wa) int32 or None).  No
    host read.  stages: a list that receives (name, ms) per stage, each after a device synchronisation."""
    _chk(vertices, torch.float32, "vertices")
    _chk(faces, torch.int32, "faces")
    dev = vertices.device
    n, m = int(vertices.shape[0]), int(faces.shape[0])
    if vertex_colors is not None:
        _chk(vertex_colors, torch.uint8, "vertex_colors")
        if tuple(vertex_colors.shape) != (n, 3):
            raise ValueError(f"bake_texture: vertex_colors ({n}, 3)")
    chunk = FUSE_MAX_VIEWS if chunk is None else chunk
    if not 1 <= int(chunk) <= FUSE_MAX_VIEWS:
        raise ValueError(f"bake_texture: chunk must be in [1, {FUSE_MAX_VIEWS}], got {chunk!r}")
    Ha, Wa = int(rows) * int(T), int(cols) * (int(T) + 1)
    vbuf = vertices if n else torch.zeros((1, 3), dtype=torch.float32, device=dev)       # n = 0: no face is read, no null pointer
    sums = torch.empty((Ha, Wa, 4), dtype=torch.float32, device=dev)                     # the first launch writes every entry
    cnt = torch.empty((Ha, Wa), dtype=torch.int32, device=dev) if count else None
    atlas = torch.empty((Ha, Wa, 3), dtype=torch.uint8, device=dev)
    L = _lib.lib()
    t_stage = [time.perf_counter()]
    totals = {}

    def stage(name):
        if stages is not None:
            torch.cuda.synchronize(dev)
            now = time.perf_counter()
            totals[name] = totals.get(name, 0.0) + 1e3 * (now - t_stage[0])
            t_stage[0] = now

    for s in range(0, max(len(views), 1), int(chunk)):
        part = views[s:s + int(chunk)]
        k = len(part)
        P = np.ascontiguousarray([np.asarray(v[0], np.float32).reshape(12) for v in part], dtype=np.float32).reshape(k, 12)
        centre = np.ascontiguousarray([np.asarray(v[1], np.float32).reshape(3) for v in part], dtype=np.float32).reshape(k, 3)
        hw = np.ascontiguousarray([tuple(v[3].shape) for v in part], dtype=np.int32).reshape(k, 2)
        stage("other")
        records = [texture_pack_view(v[2], v[3]) for v in part]
        stage("pack")
        L.surf_texture_bake(_p(vbuf), n, _p(faces), m, int(T), int(cols), int(rows), _np_ptr(P), _np_ptr(centre),
                            _ptr_array(records) if k else None, _np_ptr(hw), k, ctypes.c_float(float(z_min)),
                            ctypes.c_float(float(depth_tol)), ctypes.c_float(float(min_cos)), int(power), int(bool(two_sided)),
                            int(s == 0), _p(sums), _p(cnt), _stream())
        stage("bake")
        del records
    L.surf_texture_finish(_p(sums), n, _p(faces), m, int(T), int(cols), int(rows), _p(vertex_colors), ctypes.c_float(float(fill)),
                          _p(atlas), _stream())
    stage("finish")
    if stages is not None:
        stages.extend((k, totals[k]) for k in ("pack", "bake", "finish") if k in totals)
    return atlas, sums, cnt


MESHDIST_HOST_READS = 2         # the LEAST point_to_mesh waits for the device: one more per growth of the cell, see its docstring
MESHDIST_MAX_AXIS_CELLS = 4096   # SURF_MESHDIST_MAX_AXIS_CELLS of include/surf_hip.h
MESHDIST_MAX_CELLS = 1 << 26     # SURF_MESHDIST_MAX_CELLS
MESHDIST_PAIRS_PER_FACE = 8      # SURF_MESHDIST_PAIRS_PER_FACE
MESHDIST_MIN_PAIR_BUDGET = 1 << 16


def meshdist_cell_dims(ext, m, start_cell=None):
    """(cell, dims) of the cell table over a box of extents `ext` that holds m faces: _table_cell_dims with at most
    MESHDIST_MAX_AXIS_CELLS - 1 cells along an axis and MESHDIST_MAX_CELLS in all.  Pure host arithmetic, shared with the host path."""
    return _table_cell_dims(ext, m, max(ext) / (MESHDIST_MAX_AXIS_CELLS - 2), MESHDIST_MAX_CELLS, start_cell)


def meshdist_pair_budget(m):
    """The most (cell, face) pairs a table of m faces may list before its cell grows (include/surf_hip.h, PAIR BUDGET)."""
    return max(MESHDIST_PAIRS_PER_FACE * m, MESHDIST_MIN_PAIR_BUDGET)


def point_to_mesh(points, vertices, faces, max_dist=None, cell=None, stages=None, stats=None):
    """The surf_meshdist_* rule on device tensors: points (k, 3) fp32, vertices (n, 3) fp32, faces (m, 3) int32 -> (distance (k,)
    fp64, face (k,) int64, closest (k, 3) fp64); +inf, -1 and +inf where the distance is not < max_dist.  max_dist None: the
    diagonal of the joint bounding box of points and vertices.  The scans, sorts and gathers between the kernels are torch's.
    At least MESHDIST_HOST_READS reads of the device, each one small copy: (1) [smallest and largest face index, all vertices finite, all
    points finite, the boxes of the vertices the faces name, of the points and of the vertices] before any kernel, (2) the number
    of (cell, face) pairs, which sizes the table; read (2) is repeated once for every growth of the cell by 1.25 that the pair
    budget asks for (none where the faces are about as large as the cells or smaller; a face that spans the table can ask for
    several, at most log(MESHDIST_MAX_AXIS_CELLS) / log(1.25) = 38, after which the table is one cell).  Without a point and without a vertex
    nothing is read.  A face index outside the vertex list, a vertex or a point that is not finite raise ValueError after (1).
    cell: the cell size to use, not grown for the pair budget (tests).  stages: a list that receives (name, start event, end
    event) per stage (pairs, sort, query); stats: a dict that receives cell, dims, pairs and max_dist."""
    from .mesh_distance import check_max_dist, diagonal
    _chk(points, torch.float32, "points")
    _chk(vertices, torch.float32, "vertices")
    _chk(faces, torch.int32, "faces")
    if any(t.dim() != 2 or t.shape[1] != 3 for t in (points, vertices, faces)):
        raise ValueError(f"point_to_mesh: expected (k, 3) points, (n, 3) vertices and (m, 3) faces, got {tuple(points.shape)}, "
                         f"{tuple(vertices.shape)}, {tuple(faces.shape)}")
    max_dist = check_max_dist(max_dist)
    k, n, m, dev = points.shape[0], vertices.shape[0], faces.shape[0], points.device
    if max(k, n, m) > 2 ** 31 - 1:
        _lib.check(-2, f"point_to_mesh: {k} points / {n} vertices / {m} faces")
    distance = torch.full((k,), float("inf"), dtype=torch.float64, device=dev)
    face = torch.full((k,), -1, dtype=torch.int64, device=dev)
    closest = torch.full((k, 3), float("inf"), dtype=torch.float64, device=dev)
    if k == 0 and n == 0:
        if m:
            raise ValueError(f"face indices span [{int(faces.min())}, {int(faces.max())}], the mesh has 0 vertices")
        return distance, face, closest

    def stage(name):
        if stages is not None:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            if stages:
                stages[-1] = stages[-1][:2] + (ev,)
            if name is not None:
                stages.append((name, ev, None))

    def box(t):                                        # [lo (3), hi (3)] as fp64, zeros for an empty tensor
        return torch.cat([t.amin(0), t.amax(0)]).double() if t.shape[0] else torch.zeros(6, dtype=torch.float64, device=dev)

    stage("pairs")
    zero = torch.zeros(1, dtype=torch.float64, device=dev)
    f_range = torch.stack(torch.aminmax(faces)).double() if m else torch.cat([zero, zero])
    named = vertices[faces.reshape(-1).long().clamp_(0, max(n - 1, 0))] if m and n else vertices[:0]
    finite = torch.stack([torch.isfinite(vertices).all(), torch.isfinite(points).all()]).double()
    read = torch.cat([f_range, finite, box(named), box(points), box(vertices)]).tolist()                      # host read 1
    f_lo, f_hi = int(read[0]), int(read[1])
    if m and (f_lo < 0 or f_hi >= n):
        raise ValueError(f"face indices span [{f_lo}, {f_hi}], the mesh has {n} vertices")
    for ok, t, what in ((read[2], vertices, "vertex"), (read[3], points, "point")):
        if not ok:
            i = int(torch.nonzero(~torch.isfinite(t).all(dim=1))[0, 0])
            raise ValueError(f"point_to_mesh: {what} {i} is not finite: {t[i].tolist()}")
    if max_dist is None:
        boxes = [read[10:16]] * (k > 0) + [read[16:22]] * (n > 0)
        max_dist = diagonal([min(b[a] for b in boxes) for a in range(3)], [max(b[3 + a] for b in boxes) for a in range(3)])
    if k == 0 or m == 0:
        return distance, face, closest
    L, s = _lib.lib(), _stream()
    lo, ext = read[4:7], [b - a for a, b in zip(read[4:7], read[7:10])]
    budget = meshdist_pair_budget(m)
    c, dims = meshdist_cell_dims(ext, m, start_cell=cell)
    records = torch.empty(m, 12, dtype=torch.float32, device=dev)
    counts = torch.empty(m, dtype=torch.int64, device=dev)
    while True:
        L.surf_meshdist_pairs_count(_p(vertices), n, _p(faces), m, lo[0], lo[1], lo[2], c, dims[0], dims[1], dims[2], _p(records),
                                    _p(counts), s)
        ends = torch.cumsum(counts, 0)
        pairs = int(ends[-1])                                                                                 # host read 2
        if cell is not None or pairs <= budget:
            break
        c, dims = meshdist_cell_dims(ext, m, start_cell=1.25 * c)
    if pairs > 2 ** 31 - 1:
        _lib.check(-2, f"point_to_mesh: {pairs} (cell, face) pairs at the cell size {c}")
    ncell = dims[0] * dims[1] * dims[2]
    pair_cell = torch.empty(pairs, dtype=torch.int64, device=dev)
    pair_face = torch.empty(pairs, dtype=torch.int32, device=dev)
    L.surf_meshdist_pairs_emit(_p(records), m, lo[0], lo[1], lo[2], c, dims[0], dims[1], dims[2], _p(ends - counts), pairs,
                               _p(pair_cell), _p(pair_face), s)
    stage("sort")
    skeys, by_cell = torch.sort(pair_cell)
    per_cell = torch.zeros(ncell, dtype=torch.int64, device=dev).scatter_add_(0, skeys, torch.ones_like(skeys))   # (bincount reads)
    cstart = torch.zeros(ncell + 1, dtype=torch.int32, device=dev)
    cstart[1:] = torch.cumsum(per_cell, 0)
    cell_records = records[pair_face[by_cell].long()].contiguous()
    del pair_cell, pair_face, skeys, by_cell, per_cell
    # the queries in the order of their cells (clamped to the table): speed only, the kernel writes every query's own rows
    qc = [((points[:, a].double() - lo[a]) / c).floor_().clamp_(0.0, float(dims[a] - 1)).long() for a in range(3)]
    order = torch.sort((qc[0] * dims[1] + qc[1]) * dims[2] + qc[2])[1]
    stage("query")
    L.surf_meshdist_query(_p(points), _p(order), k, _p(cell_records), pairs, _p(cstart), lo[0], lo[1], lo[2], c, dims[0], dims[1],
                          dims[2], max_dist, _p(distance), _p(face), _p(closest), s)
    stage(None)
    if stats is not None:
        stats.update(cell=c, dims=list(dims), pairs=pairs, max_dist=max_dist)
    return distance, face, closest


def meshdist_stats(distance):
    """The statistics of one direction of the deviation rule from distance (k,) fp64 on the device, k >= 1: [found, largest
    distance, S1, S2] as Python floats (the largest is -inf with nothing found), the sums by surf_smooth_sum256.  One read."""
    _chk(distance, torch.float64, "distance")
    L, s = _lib.lib(), _stream()
    found = torch.isfinite(distance)
    d = torch.where(found, distance, torch.zeros_like(distance))
    sums = []
    for total in (d, d * d):
        while total.shape[0] > 1:                                      # the 256-ary sequential tree of the smoothing rule 4
            runs = torch.empty((total.shape[0] + 255) // 256, dtype=torch.float64, device=distance.device)
            L.surf_smooth_sum256(_p(total), total.shape[0], _p(runs), s)
            total = runs
        sums.append(total[0])
    largest = torch.where(found, distance, torch.full_like(distance, float("-inf"))).max()
    return torch.stack([found.sum().double(), largest] + sums).tolist()


# ------------------------------------------------------------------------------------------------
# the DTU protocol's mesh cleaner (dtu_clean.hip): elliptical dilation, rounded projection into padded masks, vertex removal
# ------------------------------------------------------------------------------------------------


def dtu_clean_dilate(masks, half_widths):
    """Maximum of every (h, w) slice of masks (nv, h, w) uint8 over the footprint whose row i covers the columns
    [-half_widths[i], half_widths[i]] (clean_dtu.dilate_ellipse with clean_dtu.ellipse_half_widths); returns uint8."""
    _chk(masks, torch.uint8, "masks")
    assert masks.dim() == 3
    half = [int(x) for x in half_widths]
    if len(half) % 2 == 0 or len(half) > 64:
        raise ValueError("the footprint needs an odd number of rows, at most 63")
    out = torch.empty_like(masks)
    if masks.numel():
        nv, h, w = masks.shape
        hw = torch.tensor(half, dtype=torch.int32).to(masks.device)
        _lib.lib().surf_dtu_clean_dilate(_p(masks), nv, h, w, _p(hw), len(half), _p(out), _stream())
    return out


def dtu_clean_points_in_masks(vertices, dilated, proj):
    """clean_dtu.points_in_masks on the device: per-vertex number of views whose padded mask holds the vertex, int32.
    vertices (n, 3) float64, dilated (nv, h, w) uint8 (set where > 128) on the device; proj (nv, 4, 4) or (nv, 3, 4) float32,
    host or device."""
    _chk(vertices, torch.float64, "vertices")
    _chk(dilated, torch.uint8, "dilated")
    nv, h, w = dilated.shape
    n = vertices.shape[0]
    count = torch.zeros(n, dtype=torch.int32, device=vertices.device)
    if n == 0 or nv == 0:
        return count
    P = torch.as_tensor(proj)
    if P.dtype != torch.float32 or P.shape[0] != nv or tuple(P.shape[1:]) not in ((4, 4), (3, 4)):
        raise TypeError("proj: expected (n_views, 4, 4) or (n_views, 3, 4) float32")
    P = P[:, :3, :].contiguous().to(vertices.device)
    _lib.lib().surf_dtu_clean_points_in_masks(_p(vertices), n, _p(dilated), _p(P), nv, h, w, _p(count), _stream())
    return count


def dtu_clean_remove_vertices(vertices, faces, count, minimal_vis):
    """clean_dtu.clean_faces_by_mask on the device: the vertices with count > minimal_vis in their order (referenced or not) and
    the faces whose three vertices are kept, renumbered.  vertices (V, 3) of a 4- or 8-byte dtype, faces (F, 3) int32, count
    (V,) int32.  Returns (vertices, faces, the (V,) bool vertex flags).  One host read (the two counts)."""
    _chk(faces, torch.int32, "faces")
    _chk(count, torch.int32, "count")
    if not torch.is_tensor(vertices) or not vertices.is_contiguous() or vertices.element_size() not in (4, 8):
        raise TypeError("vertices: expected a contiguous tensor of a 4- or 8-byte dtype")
    nf, nv, dev = faces.shape[0], vertices.shape[0], vertices.device
    if count.shape[0] != nv:
        raise ValueError("count: expected one entry per vertex")
    if nv == 0:
        return vertices[:0], faces[:0], torch.zeros(0, dtype=torch.bool, device=dev)
    L = _lib.lib()
    vkeep = torch.empty(nv, dtype=torch.uint8, device=dev)
    fkeep = torch.empty(nf, dtype=torch.uint8, device=dev)
    L.surf_dtu_clean_keep(_p(count), nv, _p(faces) if nf else None, nf, int(minimal_vis), _p(vkeep),
                          _p(fkeep) if nf else None, _stream())
    vscan = torch.cumsum(vkeep, 0, dtype=torch.int64)
    fscan = torch.cumsum(fkeep, 0, dtype=torch.int64)
    n_v, n_f = (int(x) for x in torch.stack([vscan[-1], fscan[-1] if nf else torch.zeros_like(vscan[-1])]).tolist())
    out_v = torch.empty(n_v, 3, dtype=vertices.dtype, device=dev)
    out_f = torch.empty(n_f, 3, dtype=torch.int32, device=dev)
    if n_v:
        L.surf_clean_compact_rows(_p(vertices), vertices.element_size(), _p(vkeep), _p(vscan), nv, _p(out_v), _stream())
    if n_f:
        L.surf_clean_compact_faces(_p(faces), _p(fkeep), _p(fscan), _p(vscan), nf, nv, _p(out_f), _stream())
    return out_v, out_f, vkeep.view(torch.bool)


# ------------------------------------------------------------------------------------------------
# per-scene fine-tuning (finetune_rays.hip): the ray batch of one view, made on the device
# ------------------------------------------------------------------------------------------------


def finetune_rays(px, py, kinv, c2w, image, depth=None):
    """Rays of one view through pixel coordinates (px, py) ((R,) device tensors, both fp32 or both int32).  kinv: (9,) fp32
    device, inverse(K)[:3, :3] row-major; c2w: (12,) fp32 device, c2w[:3, :4] row-major; image (h, w, 3) fp32, depth (h, w) fp32
    or None.  Returns rays_o, rays_d, color (R, 3) and pseudo_depth (R,) or None; color / pseudo_depth are the texels at
    (long(py), long(px)).  The fp32 operation order is the one written out in finetune_rays.hip."""
    if px.dtype not in (torch.float32, torch.int32) or py.dtype != px.dtype:
        raise TypeError("px, py: expected two fp32 or two int32 tensors")
    _chk(px, px.dtype, "px")
    _chk(py, py.dtype, "py")
    _chk(kinv, torch.float32, "kinv")
    _chk(c2w, torch.float32, "c2w")
    _chk(image, torch.float32, "image")
    if depth is not None:
        _chk(depth, torch.float32, "depth")
    if px.dim() != 1 or py.shape != px.shape or kinv.numel() != 9 or c2w.numel() != 12 or image.dim() != 3 or image.shape[2] != 3 \
            or (depth is not None and tuple(depth.shape) != tuple(image.shape[:2])):
        raise ValueError("finetune_rays: px / py (R,), kinv (9,), c2w (12,), image (h, w, 3), depth (h, w)")
    n, dev = int(px.shape[0]), px.device
    h, w = int(image.shape[0]), int(image.shape[1])
    rays_o = torch.empty(n, 3, dtype=torch.float32, device=dev)
    rays_d = torch.empty(n, 3, dtype=torch.float32, device=dev)
    color = torch.empty(n, 3, dtype=torch.float32, device=dev)
    pseudo = torch.empty(n, dtype=torch.float32, device=dev) if depth is not None else None
    if n:
        _lib.lib().surf_finetune_rays(_p(px), _p(py), int(px.dtype == torch.int32), n, _p(kinv), _p(c2w), _p(image),
                                      _p(depth), h, w, _p(rays_o), _p(rays_d), _p(color), _p(pseudo), _stream())
    return rays_o, rays_d, color, pseudo


def finetune_gather_pts(pts, idx):
    """pts[idx] for pts (N, 3) fp32 and idx (M,) int32 on the device."""
    _chk(pts, torch.float32, "pts")
    _chk(idx, torch.int32, "idx")
    if pts.dim() != 2 or pts.shape[1] != 3 or idx.dim() != 1:
        raise ValueError("finetune_gather_pts: pts (N, 3), idx (M,)")
    out = torch.empty(idx.shape[0], 3, dtype=torch.float32, device=pts.device)
    if idx.shape[0]:
        _lib.lib().surf_finetune_gather_pts(_p(pts), pts.shape[0], _p(idx), idx.shape[0], _p(out), _stream())
    return out


# ------------------------------------------------------------------------------------------------
# generalisation training (train_batch.hip): the batch of one item from the device-resident training set
# ------------------------------------------------------------------------------------------------


def _chk_plane(t, dtype, shape, name):
    _chk(t, dtype, name)
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
    if t.data_ptr() % 4:
        raise ValueError(f"{name}: expected a 4-byte aligned tensor")
    return t


def train_views(images, masks, depths, pseudos, scale):
    """The per-view planes of one training item.  images: 1..SURF_MAX_VIEWS uint8 (h, w, 3) device tensors, one per view slot (a
    tensor may repeat); masks / depths / pseudos: two uint8 (h, w) 0/1 masks and two + two fp32 (h, w) unscaled depth maps, those
    of the reference view and of the supervised source view.  Returns imgs (V, 3, h, w) = texel / 256, masks (2, h, w) fp32 and
    depths, pseudo depths (2, h, w) = (float)((double)d * scale), the host reader's rounding (train_batch.hip)."""
    images, masks, depths, pseudos = list(images), list(masks), list(depths), list(pseudos)
    if not images or len(masks) != 2 or len(depths) != 2 or len(pseudos) != 2:
        raise ValueError("train_views: at least one image; two masks, two depth maps, two pseudo depth maps")
    if images[0].dim() != 3:
        raise ValueError("train_views: images (h, w, 3)")
    h, w = int(images[0].shape[0]), int(images[0].shape[1])
    for i, t in enumerate(images):
        _chk_plane(t, torch.uint8, (h, w, 3), f"images[{i}]")
    for j in range(2):
        _chk_plane(masks[j], torch.uint8, (h, w), f"masks[{j}]")
        _chk_plane(depths[j], torch.float32, (h, w), f"depths[{j}]")
        _chk_plane(pseudos[j], torch.float32, (h, w), f"pseudos[{j}]")
    dev = images[0].device
    imgs = torch.empty(len(images), 3, h, w, dtype=torch.float32, device=dev)
    mask_out, depth_out, pseudo_out = (torch.empty(2, h, w, dtype=torch.float32, device=dev) for _ in range(3))
    _lib.lib().surf_train_views(_ptr_array(images), len(images), h, w, _ptr_array(masks), _ptr_array(depths), _ptr_array(pseudos),
                                float(scale), _p(imgs), _p(mask_out), _p(depth_out), _p(pseudo_out), _stream())
    return imgs, mask_out, depth_out, pseudo_out


def train_rays(pick, free_x, free_y, inside, kinv, c2w, image, mask, depth, pseudo, scale):
    """The ray block of one training item: len(pick) + len(free_x) rays of the reference view, masked pixels first.  pick (n_masked,)
    int32 indices into `inside` (n_inside,) int32, the row-major flat indices of the pixels inside the mask; free_x / free_y
    (n_free,) int32 with n_free = n_rays // 4 - all on the device.  kinv (9 values) = inverse(K)[:3, :3], c2w (12 values) =
    c2w[:3, :4]: fp32 HOST tensors or arrays.  image (h, w, 3) uint8, mask (h, w) uint8, depth / pseudo (h, w) fp32 unscaled.
    Returns a dict with pixels_x, pixels_y, rays_o, rays_d, color, depth, pseudo_depth, mask.  The fp32 operation order is the one
    written out in train_batch.hip."""
    for t, name in ((pick, "pick"), (free_x, "free_x"), (free_y, "free_y"), (inside, "inside")):
        _chk(t, torch.int32, name)
        if t.dim() != 1:
            raise ValueError(f"train_rays: {name} is a vector")
    n_masked, n_free = int(pick.shape[0]), int(free_x.shape[0])
    n = n_masked + n_free
    if free_y.shape != free_x.shape or n_free != n // 4 or n == 0 or inside.shape[0] == 0:
        raise ValueError("train_rays: len(free_x) == len(free_y) == n_rays // 4, n_rays = len(pick) + len(free_x) > 0, inside not empty")
    if image.dim() != 3:
        raise ValueError("train_rays: image (h, w, 3)")
    h, w = int(image.shape[0]), int(image.shape[1])
    _chk_plane(image, torch.uint8, (h, w, 3), "image")
    _chk_plane(mask, torch.uint8, (h, w), "mask")
    _chk_plane(depth, torch.float32, (h, w), "depth")
    _chk_plane(pseudo, torch.float32, (h, w), "pseudo")
    kinv = np.ascontiguousarray(np.asarray(kinv, dtype=np.float32).reshape(-1))
    c2w = np.ascontiguousarray(np.asarray(c2w, dtype=np.float32).reshape(-1))
    if kinv.size != 9 or c2w.size != 12:
        raise ValueError("train_rays: kinv (9 values), c2w (12 values)")
    dev = image.device
    new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)                    # noqa: E731
    out = {"pixels_x": new(n), "pixels_y": new(n), "rays_o": new(n, 3), "rays_d": new(n, 3), "color": new(n, 3), "depth": new(n),
           "pseudo_depth": new(n), "mask": new(n)}
    _lib.lib().surf_train_rays(_p(pick), _p(free_x) if n_free else None, _p(free_y) if n_free else None, n, _p(inside),
                               int(inside.shape[0]), _np_ptr(kinv), _np_ptr(c2w), _p(image), _p(mask), _p(depth), _p(pseudo),
                               float(scale), h, w, _p(out["pixels_x"]), _p(out["pixels_y"]), _p(out["rays_o"]), _p(out["rays_d"]),
                               _p(out["color"]), _p(out["depth"]), _p(out["pseudo_depth"]), _p(out["mask"]), _stream())
    return out


# ------------------------------------------------------------------------------------------------
# per-vertex mesh attributes (vertex_attrs.hip): the stages around sdf_mlp / blend over a vertex list
# ------------------------------------------------------------------------------------------------


def vertex_points(vertices):
    """Mesh vertices (V, 3), float64 or fp32 on the device -> (pts (V, 3) fp32, idx (V,) int32 = 0 .. V-1): the point rows and the
    identity index list sdf_mlp / blend take as active_idx.  float64 -> fp32 rounds to nearest, as torch.Tensor.float()."""
    if not torch.is_tensor(vertices) or vertices.dtype not in (torch.float64, torch.float32):
        raise TypeError("vertices: expected a float64 or float32 tensor")
    _chk(vertices, vertices.dtype, "vertices")
    if vertices.dim() != 2 or vertices.shape[1] != 3:
        raise ValueError("vertex_points: vertices (V, 3)")
    n, dev = int(vertices.shape[0]), vertices.device
    pts = torch.empty(n, 3, dtype=torch.float32, device=dev)
    idx = torch.empty(n, dtype=torch.int32, device=dev)
    if n:
        _lib.lib().surf_vertex_points(_p(vertices), int(vertices.dtype == torch.float64), n, _p(pts), _p(idx), _stream())
    return pts, idx


def vertex_finish(grad, color, n_valid, normals=None, colors=None):
    """SDF gradients (V, 3) fp32, blend colours (V, 3) fp32 and view counts (V,) uint8 -> (normals (V, 3) fp32 = grad / |grad|,
    zero rows where |grad| is 0 or not finite; colors (V, 3) uint8 = trunc(clamp(color * 256, 0, 255)), grey 128 where n_valid is
    0).  normals / colors: optional outputs to write into.  The fp32 operation order is the one written out in vertex_attrs.hip."""
    _chk(grad, torch.float32, "grad")
    _chk(color, torch.float32, "color")
    _chk(n_valid, torch.uint8, "n_valid")
    n, dev = int(n_valid.shape[0]), grad.device
    if tuple(grad.shape) != (n, 3) or tuple(color.shape) != (n, 3) or n_valid.dim() != 1:
        raise ValueError("vertex_finish: grad (V, 3), color (V, 3), n_valid (V,)")
    normals = torch.empty(n, 3, dtype=torch.float32, device=dev) if normals is None else _chk(normals, torch.float32, "normals")
    colors = torch.empty(n, 3, dtype=torch.uint8, device=dev) if colors is None else _chk(colors, torch.uint8, "colors")
    if tuple(normals.shape) != (n, 3) or tuple(colors.shape) != (n, 3):
        raise ValueError("vertex_finish: normals (V, 3), colors (V, 3)")
    if n:
        _lib.lib().surf_vertex_finish(_p(grad), _p(color), _p(n_valid), n, _p(normals), _p(colors), _stream())
    return normals, colors


def vertex_scratch_bytes(n, nv, sdf_precision, blend_precision):
    """Device scratch the SDF gradient kernel and the blend kernel take for a launch over n points (their scratch-bytes queries)."""
    L = _lib.lib()
    fn = "surf_sdf_scratch_bytes" if sdf_precision == "f32" else f"surf_sdf_{_SPLIT_ABI[sdf_precision]}_scratch_bytes"
    need = int(getattr(L, fn)(int(n)))
    if blend_precision != "f32":
        need += int(L.surf_blend_split_scratch_bytes(int(n), int(nv)))
    return need


def marching_cubes(u, isovalue=0.0, observed_only=False):
    """mcubes.marching_cubes(u, isovalue) (implicit_surface.py:353) on a device lattice u (nx, ny, nz) fp32.
    Returns (vertices (nv, 3) float64, triangles (nt, 3) int32) device tensors, vertices in lattice-index units.
    Two host syncs size the outputs (number of active lattice points, then vertex / triangle totals).
    observed_only (ours, for fused lattices: NaN = no view saw the point): surf_mc_classify_observed instead of surf_mc_classify -
    vertices only on edges with two finite end points, triangles only in cells with eight finite corners - and the vertices that
    no triangle references (an edge none of whose cells is fully observed) dropped through clean_update_faces."""
    _chk(u, torch.float32, "u")
    assert u.dim() == 3
    nx, ny, nz = (int(v) for v in u.shape)
    dev = u.device
    L = _lib.lib()
    flags = torch.empty(nx * ny * nz, dtype=torch.uint8, device=dev)
    iso = ctypes.c_double(float(isovalue))       # PyMCubes takes the isovalue as a double
    (L.surf_mc_classify_observed if observed_only else L.surf_mc_classify)(_p(u), nx, ny, nz, iso, _p(flags), _stream())
    active = compact(flags)
    m = int(active.shape[0])
    if m == 0:
        return torch.zeros(0, 3, dtype=torch.float64, device=dev), torch.zeros(0, 3, dtype=torch.int32, device=dev)
    ws = torch.empty(L.surf_mc_workspace_ints(m), dtype=torch.int32, device=dev)
    totals = torch.empty(2, dtype=torch.int32, device=dev)
    L.surf_mc_count(_p(flags), _p(active), m, _p(ws), _p(totals), _stream())
    n_v, n_t = (int(v) for v in totals.tolist())
    vertices = torch.empty(n_v, 3, dtype=torch.float64, device=dev)
    triangles = torch.empty(n_t, 3, dtype=torch.int32, device=dev)
    vbase = torch.empty(nx * ny * nz, dtype=torch.int32, device=dev)
    L.surf_mc_emit(_p(u), nx, ny, nz, iso, _p(flags), _p(active), m, _p(ws), _p(vbase), _p(vertices), _p(triangles), _stream())
    if observed_only:
        return clean_update_faces(vertices, triangles, torch.ones(n_t, dtype=torch.uint8, device=dev))
    return vertices, triangles


# ------------------------------------------------------------------------------------------------
# depth-map fusion (fuse.hip): TSDF integration of rendered depth maps into one world-frame lattice (surf_amd/fusion.py)
# ------------------------------------------------------------------------------------------------

FUSE_MAX_VIEWS = 16                              # SURF_FUSE_MAX_VIEWS: views per launch of surf_fuse_integrate


def _chk_dense_state(tsdf, weight, color, what):
    _chk(tsdf, torch.float32, "tsdf")
    _chk(weight, torch.float32, "weight")
    if tsdf.dim() != 3 or weight.shape != tsdf.shape:
        raise ValueError(f"{what}: tsdf and weight (nx, ny, nz)")
    if color is not None:
        _chk(color, torch.float32, "color")
        if tuple(color.shape) != tuple(tsdf.shape) + (3,):
            raise ValueError(f"{what}: color (nx, ny, nz, 3)")


def _chk_fuse_state(tsdf, weight, color, axes):
    _chk_dense_state(tsdf, weight, color, "fuse")
    if len(axes) != 3:
        raise ValueError("fuse: three axis arrays")
    for a, n, name in zip(axes, tsdf.shape, ("ax", "ay", "az")):
        _chk(a, torch.float32, name)
        if tuple(a.shape) != (int(n),):
            raise ValueError(f"fuse: {name} holds {tuple(a.shape)} coordinates for {int(n)} lattice points")


def _pack_fuse_views(views, color, what):
    """The host arrays of a launch's view table, (P (n, 12) fp32, hw (n, 2) int32, dscale (n,) fp32, depths, images): images is
    empty unless colours are fused (color is not None); `what` names the caller in the messages."""
    n = len(views)
    P = np.empty((n, 12), dtype=np.float32)
    hw = np.empty((n, 2), dtype=np.int32)
    dscale = np.empty(n, dtype=np.float32)
    depths, images = [], []
    for v, (Pv, depth, ds, image) in enumerate(views):
        _chk(depth, torch.float32, f"views[{v}].depth")
        if depth.dim() != 2:
            raise ValueError(f"{what}: views[{v}].depth (H, W)")
        P[v] = np.asarray(Pv, dtype=np.float32).reshape(12)
        hw[v] = depth.shape
        dscale[v] = ds
        depths.append(depth)
        if color is not None:
            if image is None:
                raise ValueError(f"{what}: colours are fused but views[{v}] has no image")
            _chk(image, torch.float32, f"views[{v}].image")
            if tuple(image.shape) != tuple(depth.shape) + (3,):
                raise ValueError(f"{what}: views[{v}].image (H, W, 3)")
            images.append(image)
    return P, hw, dscale, depths, images


def fuse_integrate(tsdf, weight, color, axes, views, trunc):
    """One launch of surf_fuse_integrate: the state tsdf / weight (nx, ny, nz) (and color (nx, ny, nz, 3), or None) is updated in
    place with `views`, at most FUSE_MAX_VIEWS of them, in order.  axes: the three device coordinate arrays of the lattice; a view
    is (P (12,) or (3, 4) fp32 on the host, depth (H, W) fp32 device tensor, dscale, image (H, W, 3) fp32 device tensor or None);
    trunc: world units.  The fp32 update sequence is written out in fuse.hip's header comment."""
    _chk_fuse_state(tsdf, weight, color, axes)
    n = len(views)
    if n == 0:
        return
    P, hw, dscale, depths, images = _pack_fuse_views(views, color, "fuse_integrate")
    nx, ny, nz = (int(v) for v in tsdf.shape)
    _lib.lib().surf_fuse_integrate(_p(tsdf), _p(weight), _p(color), _p(axes[0]), _p(axes[1]), _p(axes[2]), nx, ny, nz, _np_ptr(P),
                                   _ptr_array(depths), _ptr_array(images) if images else None, _np_ptr(hw), _np_ptr(dscale), n,
                                   ctypes.c_float(float(trunc)), _stream())


def fuse_lattice(tsdf, weight):
    """Marching cubes' input of a fused lattice: u = -tsdf where weight > 0, NaN where no view saw the point."""
    _chk(tsdf, torch.float32, "tsdf")
    _chk(weight, torch.float32, "weight")
    if weight.shape != tsdf.shape:
        raise ValueError("fuse_lattice: tsdf and weight of one shape")
    u = torch.empty_like(tsdf)
    if tsdf.numel():
        _lib.lib().surf_fuse_lattice(_p(tsdf), _p(weight), tsdf.numel(), _p(u), _stream())
    return u


def fuse_vertex_colors(vertices, color):
    """Colours (V, 3) uint8 of mesh vertices (V, 3) float64 in lattice-index units (marching_cubes' output) from the fused colour
    lattice (nx, ny, nz, 3): interpolated along the lattice edge the vertex lies on, quantised like vertex_finish's colours."""
    _chk(vertices, torch.float64, "vertices")
    _chk(color, torch.float32, "color")
    if vertices.dim() != 2 or vertices.shape[1] != 3 or color.dim() != 4 or color.shape[3] != 3:
        raise ValueError("fuse_vertex_colors: vertices (V, 3), color (nx, ny, nz, 3)")
    n = int(vertices.shape[0])
    out = torch.empty(n, 3, dtype=torch.uint8, device=vertices.device)
    if n:
        nx, ny, nz = (int(v) for v in color.shape[:3])
        _lib.lib().surf_fuse_vertex_colors(_p(vertices), n, _p(color), nx, ny, nz, _p(out), _stream())
    return out


# ---- brick-sparse fusion (fuse_sparse.hip): the same state in the 8^3-point bricks near the measured surfaces only ----

def fuse_brick_dims(shape):
    """(res, nbp) of a lattice (nx, ny, nz) in the band layout: the side of the cube it is embedded in (its longest axis) and the
    bricks per axis of that cube's table (nbp^3 entries, brick ids (bx nbp + by) nbp + bz)."""
    res = max(int(n) for n in shape)
    return res, (res + 7) // 8


def _chk_fuse_axes(axes):
    if len(axes) != 3:
        raise ValueError("fuse: three axis arrays")
    for a, name in zip(axes, ("ax", "ay", "az")):
        _chk(a, torch.float32, name)
        if a.dim() != 1 or a.numel() < 1:
            raise ValueError(f"fuse: {name} is a 1-d array of coordinates")
    return tuple(int(a.numel()) for a in axes)


def fuse_mark_bricks(mark, axes, lift, depth, dscale, trunc):
    """One view's marks: mark (nbp^3 bytes of the lattice's brick table, see fuse_brick_dims) gets a 1 at every brick that can
    hold a lattice point the view updates within the truncation distance, or a neighbour of one - a conservative superset, the
    rule is written out in fuse_sparse.hip's header comment.  axes: the three device coordinate arrays, strictly increasing;
    lift: fusion.lift_transform(view) (12 fp32 on the host); depth (H, W) fp32 device tensor."""
    nx, ny, nz = _chk_fuse_axes(axes)
    _chk(mark, torch.uint8, "mark")
    _chk(depth, torch.float32, "depth")
    if depth.dim() != 2:
        raise ValueError("fuse_mark_bricks: depth (H, W)")
    if mark.numel() != fuse_brick_dims((nx, ny, nz))[1] ** 3:
        raise ValueError("fuse_mark_bricks: mark holds one byte per brick of the table")
    if depth.numel() == 0:
        return
    lift = np.ascontiguousarray(np.asarray(lift, dtype=np.float32).reshape(12))
    H, W = (int(v) for v in depth.shape)
    _lib.lib().surf_fuse_mark_bricks(_p(depth), H, W, ctypes.c_float(float(dscale)), _np_ptr(lift), _p(axes[0]), _p(axes[1]),
                                     _p(axes[2]), nx, ny, nz, ctypes.c_float(float(trunc)), _p(mark), _stream())


def fuse_assign_bricks(mark):
    """(table (nbp^3,) int32: brick id -> slot or -1, bricks (n_slots,) int32: the marked brick ids, ascending) of a mark array;
    the marks are cleared.  One host read (the count)."""
    _chk(mark, torch.uint8, "mark")
    ids = compact(mark)
    m = int(ids.shape[0])
    table = torch.full((mark.numel(),), -1, dtype=torch.int32, device=mark.device)
    bricks = torch.empty(m, dtype=torch.int32, device=mark.device)
    if m:
        _lib.lib().surf_band_assign(_p(ids), m, 0, _p(table), _p(bricks), _p(mark), _stream())
    return table, bricks


def _chk_brick_state(tsdf, weight, color, m, what):
    """Brick-major state of m bricks: tsdf / weight (m * 512,) and color (m * 512, 3) or None."""
    _chk(tsdf, torch.float32, "tsdf")
    _chk(weight, torch.float32, "weight")
    if tsdf.numel() != m * 512 or weight.numel() != m * 512:
        raise ValueError(f"{what}: tsdf and weight hold 512 points per brick")
    if color is not None:
        _chk(color, torch.float32, "color")
        if color.numel() != m * 512 * 3:
            raise ValueError(f"{what}: color holds 512 x 3 values per brick")


def _chk_brick_table(table, shape, what):
    _chk(table, torch.int32, "table")
    if table.numel() != fuse_brick_dims(shape)[1] ** 3:
        raise ValueError(f"{what}: table holds one entry per brick")


def fuse_integrate_bricks(tsdf, weight, color, bricks, axes, views, trunc):
    """fuse_integrate on brick-major state: tsdf / weight (n_slots * 512,) and color (n_slots * 512, 3) or None are updated in
    place with `views` (fuse_integrate's tuples, at most FUSE_MAX_VIEWS, in order) at every lattice point of the listed bricks;
    points past the upper faces are never updated.  The per-point arithmetic is fuse.hip's."""
    nx, ny, nz = _chk_fuse_axes(axes)
    _chk(bricks, torch.int32, "bricks")
    m = int(bricks.shape[0])
    _chk_brick_state(tsdf, weight, color, m, "fuse_integrate_bricks")
    n = len(views)
    if n == 0 or m == 0:
        return
    P, hw, dscale, depths, images = _pack_fuse_views(views, color, "fuse_integrate_bricks")
    _lib.lib().surf_fuse_integrate_bricks(_p(tsdf), _p(weight), _p(color), _p(bricks), m, _p(axes[0]), _p(axes[1]), _p(axes[2]), nx,
                                          ny, nz, _np_ptr(P), _ptr_array(depths), _ptr_array(images) if images else None,
                                          _np_ptr(hw), _np_ptr(dscale), n, ctypes.c_float(float(trunc)), _stream())


def fuse_band_values(tsdf, weight):
    """The band values of brick-major state: u = -tsdf where weight > 0, NaN elsewhere (fuse_lattice on the flat arrays)."""
    return fuse_lattice(tsdf.reshape(-1), weight.reshape(-1))


def fuse_vertex_colors_bricks(vertices, color, table, shape):
    """fuse_vertex_colors on brick-major colours (n_slots * 512, 3) of the lattice `shape`, read through the brick table."""
    _chk(vertices, torch.float64, "vertices")
    _chk(color, torch.float32, "color")
    _chk(table, torch.int32, "table")
    if vertices.dim() != 2 or vertices.shape[1] != 3 or color.dim() != 2 or color.shape[1] != 3:
        raise ValueError("fuse_vertex_colors_bricks: vertices (V, 3), color (n_slots * 512, 3)")
    nx, ny, nz = (int(v) for v in shape)
    _chk_brick_table(table, shape, "fuse_vertex_colors_bricks")
    n = int(vertices.shape[0])
    out = torch.empty(n, 3, dtype=torch.uint8, device=vertices.device)
    if n:
        _lib.lib().surf_fuse_vertex_colors_bricks(_p(vertices), n, _p(color), _p(table), nx, ny, nz, _p(out), _stream())
    return out


# ---- ray casting of the fused state (ray_cast.hip): depth, normal and colour of the model from any camera ----

def _ray_cast_outputs(hw, color, normals, dev):
    H, W = (int(v) for v in hw)
    if H < 0 or W < 0:
        raise ValueError("fuse_ray_cast: hw = (H, W), both >= 0")
    depth = torch.empty(H, W, dtype=torch.float32, device=dev)
    normal = torch.empty(H, W, 3, dtype=torch.float32, device=dev) if normals else None
    out_color = None if color is None else torch.empty(H, W, 3, dtype=torch.float32, device=dev)
    return H, W, depth, normal, out_color


def fuse_ray_cast(tsdf, weight, color, lift, hw, z_min=0.0, level=0.0, normals=True):
    """The dense state tsdf / weight (nx, ny, nz) (and color (nx, ny, nz, 3) or None) of a UNIFORM lattice seen from one camera:
    (depth (H, W), normal (H, W, 3) or None, color (H, W, 3) or None) fp32 device tensors.  lift: fusion.ray_lift(P, lo, voxel)
    (12 fp32 on the host, lattice-index units); level = -isovalue.  The rule is written out in ray_cast.hip's header comment."""
    _chk_dense_state(tsdf, weight, color, "fuse_ray_cast")
    lift = np.ascontiguousarray(np.asarray(lift, dtype=np.float32).reshape(12))
    H, W, depth, normal, out_color = _ray_cast_outputs(hw, color, normals, tsdf.device)
    nx, ny, nz = (int(v) for v in tsdf.shape)
    _lib.lib().surf_fuse_ray_cast(_p(tsdf), _p(weight), _p(color), nx, ny, nz, _np_ptr(lift), H, W, ctypes.c_float(float(z_min)),
                                  ctypes.c_float(float(level)), _p(depth), _p(normal), _p(out_color), _stream())
    return depth, normal, out_color


def fuse_ray_cast_bricks(tsdf, weight, color, table, shape, lift, hw, z_min=0.0, level=0.0, normals=True):
    """fuse_ray_cast on brick-major state (tsdf / weight (n_slots * 512,), color (n_slots * 512, 3) or None) of the lattice `shape`,
    read through the brick table: a corner in a brick that is not allocated is unobserved.  Equal arrays."""
    _chk(tsdf, torch.float32, "tsdf")
    m = tsdf.numel() // 512
    _chk_brick_state(tsdf, weight, color, m, "fuse_ray_cast_bricks")
    nx, ny, nz = (int(v) for v in shape)
    _chk_brick_table(table, shape, "fuse_ray_cast_bricks")
    lift = np.ascontiguousarray(np.asarray(lift, dtype=np.float32).reshape(12))
    H, W, depth, normal, out_color = _ray_cast_outputs(hw, color, normals, table.device)
    if m == 0:                                                     # nothing allocated: nothing is observed, no ray hits
        return depth.zero_(), None if normal is None else normal.zero_(), None if out_color is None else out_color.zero_()
    _lib.lib().surf_fuse_ray_cast_bricks(_p(tsdf), _p(weight), _p(color), _p(table), m, nx, ny, nz, _np_ptr(lift), H, W,
                                         ctypes.c_float(float(z_min)), ctypes.c_float(float(level)), _p(depth), _p(normal),
                                         _p(out_color), _stream())
    return depth, normal, out_color


# ------------------------------------------------------------------------------------------------
# multi-view geometric consistency of depth maps (depth_filter.hip): which pixels do enough other views agree with
# ------------------------------------------------------------------------------------------------

# the pixels one wavefront covers: 64 (flat index), 16 (x 4) or 8 (x 8).  16 x 4 and 8 x 8 measure alike, 64 x 1 is 9-15 % slower
# at 16 sources from 576 x 800 up (profiles/depth_filter.txt)
DEPTH_FILTER_TILE_W = 16


def _chk_consistency_state(depth, count, zsum, what):
    _chk(depth, torch.float32, f"{what}: ref depth")
    _chk(count, torch.int32, f"{what}: count")
    _chk(zsum, torch.float32, f"{what}: zsum")
    if depth.dim() != 2 or count.shape != depth.shape or zsum.shape != depth.shape:
        raise ValueError(f"{what}: ref depth, count and zsum (H, W)")
    if count.device != depth.device or zsum.device != depth.device:
        raise ValueError(f"{what}: ref depth, count and zsum on one device")


def _consistency_sources(sources, depth_r, what):
    """The host arrays of a launch's source table: (T (n, 24) fp32, hw (n, 2) int32, dscale (n) fp32, the depth tensors)."""
    n = len(sources)
    T = np.empty((n, 24), dtype=np.float32)
    hw = np.empty((n, 2), dtype=np.int32)
    dscale = np.empty(n, dtype=np.float32)
    depths = []
    for s, (Ts, depth, ds) in enumerate(sources):
        _chk(depth, torch.float32, f"sources[{s}].depth")
        if depth.dim() != 2 or depth.numel() == 0:
            raise ValueError(f"{what}: sources[{s}].depth (Hs, Ws)")
        if depth.device != depth_r.device:
            raise ValueError(f"{what}: sources[{s}].depth is not on the reference's device")
        Ts = np.concatenate([np.asarray(p, dtype=np.float32).reshape(-1) for p in Ts]) if isinstance(Ts, (tuple, list)) else \
            np.asarray(Ts, dtype=np.float32).reshape(-1)
        if Ts.shape != (24,):
            raise ValueError(f"{what}: sources[{s}] transforms hold {Ts.size} values, not A_rs, b_rs, A_sr, b_sr = 24")
        T[s] = Ts
        hw[s] = depth.shape
        dscale[s] = ds
        depths.append(depth)
    return T, hw, dscale, depths


def depth_consistency(ref, sources, count, zsum, px_thresh=1.0, rel_thresh=0.01, tile_w=None):
    """One launch of surf_depth_consistency: the reference map ref = (depth (H, W) fp32 device tensor, dscale) is tested against
    `sources`, at most FUSE_MAX_VIEWS of them, in order; count (H, W) int32 and zsum (H, W) fp32 are updated in place (a further
    call with further sources continues them).  A source is (T, depth (Hs, Ws) fp32 device tensor, dscale) with T the 24 fp32
    values (A_rs, b_rs, A_sr, b_sr) of fusion.pair_transforms(reference, source), as one array or the four.  tile_w: the
    thread-to-pixel mapping (None: DEPTH_FILTER_TILE_W; the results do not depend on it).  The fp32 operation sequence is written
    out in depth_filter.hip's header comment."""
    depth_r, dscale_r = ref
    _chk_consistency_state(depth_r, count, zsum, "depth_consistency")
    n = len(sources)
    if n == 0:
        return
    T, hw, dscale, depths = _consistency_sources(sources, depth_r, "depth_consistency")
    px = np.float32(px_thresh)
    H, W = (int(v) for v in depth_r.shape)
    _lib.lib().surf_depth_consistency(_p(depth_r), H, W, ctypes.c_float(float(dscale_r)), _np_ptr(T), _ptr_array(depths),
                                      _np_ptr(hw), _np_ptr(dscale), n, ctypes.c_float(float(px * px)),
                                      ctypes.c_float(float(np.float32(rel_thresh))), _p(count), _p(zsum),
                                      DEPTH_FILTER_TILE_W if tile_w is None else int(tile_w), _stream())


def depth_consistency_finish(ref, count, zsum, min_consistent, average=False):
    """surf_depth_consistency_finish: (out depth (H, W) fp32, keep (H, W) uint8) of the reference map ref = (depth, dscale) from the
    count / zsum that depth_consistency accumulated: keep = measured and count >= min_consistent; out = 0 where not kept, the
    input depth where kept, or with `average` the mean over the reference and its agreeing sources."""
    depth_r, dscale_r = ref
    _chk_consistency_state(depth_r, count, zsum, "depth_consistency_finish")
    if int(min_consistent) < 0:
        raise ValueError("depth_consistency_finish: min_consistent >= 0")
    out = torch.empty_like(depth_r)
    keep = torch.empty(depth_r.shape, dtype=torch.uint8, device=depth_r.device)
    if depth_r.numel():
        _lib.lib().surf_depth_consistency_finish(_p(depth_r), ctypes.c_float(float(dscale_r)), _p(count), _p(zsum), depth_r.numel(),
                                                 int(min_consistent), int(bool(average)), _p(out), _p(keep), _stream())
    return out, keep


# ------------------------------------------------------------------------------------------------
# fused point clouds (point_cloud.hip): consistent depths of many views merged into one cloud (surf_amd/fusion.py fuse_points)
# ------------------------------------------------------------------------------------------------


def points_candidates(depth, used):
    """surf_points_candidates: the depth map (H, W) fp32 with the pixels of used (H, W) uint8 != 0 set to 0 (no measurement)."""
    _chk(depth, torch.float32, "points_candidates: depth")
    _chk(used, torch.uint8, "points_candidates: used")
    if depth.dim() != 2 or used.shape != depth.shape or used.device != depth.device:
        raise ValueError("points_candidates: depth and used (H, W) on one device")
    out = torch.empty_like(depth)
    if depth.numel():
        _lib.lib().surf_points_candidates(_p(depth), _p(used), depth.numel(), _p(out), _stream())
    return out


def points_mark(ref, keep, sources, used, px_thresh=1.0, rel_thresh=0.01):
    """One launch of surf_points_mark: at the pixels of the reference map ref = (candidate depth (H, W) fp32, dscale) with
    keep (H, W) uint8 != 0 the consistency rule is re-run against `sources` (as for depth_consistency, at most FUSE_MAX_VIEWS)
    and used[s] (Hs, Ws) uint8, the used map of sources[s], gets a 1 at the pixel each agreeing source was matched at."""
    depth_r, dscale_r = ref
    _chk(depth_r, torch.float32, "points_mark: ref depth")
    _chk(keep, torch.uint8, "points_mark: keep")
    if depth_r.dim() != 2 or keep.shape != depth_r.shape or keep.device != depth_r.device:
        raise ValueError("points_mark: ref depth and keep (H, W) on one device")
    n = len(sources)
    if len(used) != n:
        raise ValueError("points_mark: one used map per source")
    if n == 0 or depth_r.numel() == 0:
        return
    T, hw, dscale, depths = _consistency_sources(sources, depth_r, "points_mark")
    for s, (u, depth) in enumerate(zip(used, depths)):
        _chk(u, torch.uint8, f"points_mark: used[{s}]")
        if u.shape != depth.shape or u.device != depth.device:
            raise ValueError(f"points_mark: used[{s}] has the shape and device of sources[{s}].depth")
    px = np.float32(px_thresh)
    H, W = (int(v) for v in depth_r.shape)
    _lib.lib().surf_points_mark(_p(depth_r), H, W, ctypes.c_float(float(dscale_r)), _p(keep), _np_ptr(T), _ptr_array(depths),
                                _ptr_array(used), _np_ptr(hw), _np_ptr(dscale), n, ctypes.c_float(float(px * px)),
                                ctypes.c_float(float(np.float32(rel_thresh))), _stream())


def points_lift(ref, count, zsum, kept, lift, view, average=True, image=None):
    """surf_points_lift: (points (n, 3) fp32, colors (n, 3) uint8 or None, origin (n, 2) int32) of the kept pixels of the
    reference map ref = (candidate depth (H, W) fp32, dscale).  kept (n,) int64: their flat indices, ascending; count / zsum:
    depth_consistency's state; lift: the 12 fp32 values M^-1 (row-major) and -M^-1 t of the view's P = [M | t] on the host;
    view: the index written to origin[:, 0]; image (H, W, 3) fp32 or None.  The fp32 operation order is written out in
    point_cloud.hip's header comment."""
    depth_r, dscale_r = ref
    _chk_consistency_state(depth_r, count, zsum, "points_lift")
    _chk(kept, torch.int64, "points_lift: kept")
    if kept.dim() != 1 or kept.device != depth_r.device:
        raise ValueError("points_lift: kept (n,) on the reference's device")
    lift = np.ascontiguousarray(np.asarray(lift, dtype=np.float32).reshape(-1))
    if lift.shape != (12,):
        raise ValueError("points_lift: lift holds M^-1 and -M^-1 t = 12 values")
    if image is not None:
        _chk(image, torch.float32, "points_lift: image")
        if tuple(image.shape) != tuple(depth_r.shape) + (3,) or image.device != depth_r.device:
            raise ValueError("points_lift: image (H, W, 3) on the reference's device")
    n, dev = int(kept.shape[0]), depth_r.device
    points = torch.empty(n, 3, dtype=torch.float32, device=dev)
    colors = None if image is None else torch.empty(n, 3, dtype=torch.uint8, device=dev)
    origin = torch.empty(n, 2, dtype=torch.int32, device=dev)
    if n:
        H, W = (int(v) for v in depth_r.shape)
        _lib.lib().surf_points_lift(_p(depth_r), H, W, ctypes.c_float(float(dscale_r)), _p(count), _p(zsum), int(bool(average)),
                                    _p(kept), n, _np_ptr(lift), _p(image), int(view), _p(points), _p(colors), _p(origin), _stream())
    return points, colors, origin


# ------------------------------------------------------------------------------------------------
# narrow-band marching cubes (mesh_band.hip): the dense mesh from the SDF in 8^3-cell bricks near the surface
# ------------------------------------------------------------------------------------------------

BAND_SPLIT_BRICKS = ((1 << 31) - 1) // 512     # bricks per launch of the split kernels' brick mode (< 2^31 points)
BAND_F32_BRICKS = (1 << 24) // 512              # bricks per point tensor of the fp32 path (sdf_grid's 2^24 points per launch)


def band_dims(resolution):
    """(bricks per axis that hold cells, bricks per axis of the brick table) of a resolution^3 lattice."""
    n = int(resolution)
    return (n - 1 + 7) // 8, (n + 7) // 8


def band_coarse_index(resolution):
    """Lattice indices of the coarse screen along one axis: 0, 8, 16, .. (one per cell brick) and resolution - 1."""
    n = int(resolution)
    return list(range(0, n - 1, 8)) + [n - 1]


def sdf_bricks(axes, volumes, packed, bricks, resolution, out, sign=-1.0):
    """out[j * 512 + l] = sign * sdf at local point l of brick bricks[j] of the resolution^3 lattice on `axes` (the lattice's
    three axis arrays): the split kernel's brick mode, values bit-equal to sdf_lattice's.  Points past the upper faces are not
    written.  Split precisions only; long lists are split into launches of < 2^31 points."""
    precision = sdf_packed_precision(packed)
    if precision == "f32":
        raise ValueError("sdf_bricks: bf16x3 / f16x2 weights only (the fp32 path evaluates band_points with sdf_mlp)")
    for ax in axes:
        _chk(ax, torch.float32, "lattice axis")
    _chk(bricks, torch.int32, "bricks")
    _chk(out, torch.float32, "brick values")
    m = int(bricks.shape[0])
    assert out.numel() >= m * 512
    name = f"surf_sdf_bricks_{precision}"
    fn = getattr(_lib.lib(), name)
    for j0 in range(0, m, BAND_SPLIT_BRICKS):
        k = min(BAND_SPLIT_BRICKS, m - j0)
        fn(_p(axes[0]), _p(axes[1]), _p(axes[2]), int(resolution), _p(bricks[j0:]), k, volumes._vp, volumes._tp, volumes._dp,
           volumes.n, _p(packed), _p(out[j0 * 512:]), float(sign), _stream())


def band_points(axes, bricks, resolution):
    """(len(bricks) * 512, 3) fp32 points of the bricks' lattice points, brick-major (the floats meshgrid of `axes` gives);
    points past the upper faces repeat the last lattice point."""
    for ax in axes:
        _chk(ax, torch.float32, "lattice axis")
    _chk(bricks, torch.int32, "bricks")
    m = int(bricks.shape[0])
    pts = torch.empty(m * 512, 3, dtype=torch.float32, device=bricks.device)
    _lib.lib().surf_band_points(_p(axes[0]), _p(axes[1]), _p(axes[2]), _p(bricks), m, int(resolution), _p(pts), _stream())
    return pts


def band_screen(uc, caxes, resolution, isovalue, margin):
    """Seed marks (brick-table bytes) of the cell bricks whose coarse corners (uc: the lattice at band_coarse_index on every axis,
    caxes: its axis values) change sign or come within margin * (brick diagonal) / 2 of the isovalue."""
    _chk(uc, torch.float32, "coarse lattice")
    for ax in caxes:
        _chk(ax, torch.float32, "coarse axis")
    L = _lib.lib()
    mark = torch.zeros(int(L.surf_band_table_size(int(resolution))), dtype=torch.uint8, device=uc.device)
    L.surf_band_screen(_p(uc), _p(caxes[0]), _p(caxes[1]), _p(caxes[2]), int(resolution), ctypes.c_double(float(isovalue)),
                       ctypes.c_double(float(margin)), _p(mark), _stream())
    return mark


class Band:
    """The evaluated narrow band of a resolution^3 lattice (mesh_band.hip's state): table (nbp^3 int32: brick id -> slot or -1),
    is_cell (nbp^3 bytes: the brick's cells are meshed), bricks (slot -> brick id), values (slot * 512 + local point: u = -sdf;
    NaN past the upper faces) and the growth statistics.  shape (fused bands only): the lattice (nx, ny, nz) embedded in the
    cube of side resolution = max(shape); such a band has no is_cell and is meshed with observed_only=True."""

    def __init__(self, resolution, table, is_cell, bricks, values, stats, shape=None):
        self.resolution, self.table, self.is_cell, self.bricks, self.values, self.stats = resolution, table, is_cell, bricks, values, stats
        self.shape = shape

    @property
    def n_slots(self):
        return int(self.bricks.shape[0])


def band_grow(resolution, isovalue, mark, evaluate):
    """The growth loop: mark (band_screen's seeds, consumed) -> Band.  evaluate(bricks (k,) int32, out (k * 512,) fp32) fills the
    values of the listed bricks.  Every pass promotes the marked bricks to cell bricks, evaluates them and their forward halo,
    and marks the bricks of every cell incident to a sign-changing edge of their cells; it ends when a pass finds no new cell
    brick.  One host read per pass (the two counts)."""
    L = _lib.lib()
    dev = mark.device
    n = int(resolution)
    nt = int(L.surf_band_table_size(n))
    _chk(mark, torch.uint8, "mark")
    assert mark.numel() == nt
    iso = ctypes.c_double(float(isovalue))
    table = torch.full((nt,), -1, dtype=torch.int32, device=dev)
    is_cell = torch.zeros(nt, dtype=torch.uint8, device=dev)
    need = torch.zeros(nt, dtype=torch.uint8, device=dev)
    ws = torch.empty(L.surf_compact_workspace_ints(nt), dtype=torch.int32, device=dev)
    new_cell = torch.empty(nt, dtype=torch.int32, device=dev)
    new_eval = torch.empty(nt, dtype=torch.int32, device=dev)
    counts = torch.empty(2, dtype=torch.int32, device=dev)
    cap = 1024
    bricks = torch.empty(cap, dtype=torch.int32, device=dev)
    values = torch.full((cap * 512,), float("nan"), dtype=torch.float32, device=dev)
    n_slots, passes, seeded, grown = 0, 0, 0, 0
    for _ in range(nt + 1):                       # every pass but the last adds a cell brick
        st = _stream()
        L.surf_band_promote(_p(mark), _p(is_cell), _p(table), _p(need), n, st)
        L.surf_compact(_p(mark), nt, _p(ws), _p(new_cell), _p(counts), st)
        L.surf_compact(_p(need), nt, _p(ws), _p(new_eval), _p(counts[1:]), st)
        n_cell, n_eval = (int(v) for v in counts.tolist())            # the pass's one host read
        if n_cell == 0:
            break
        if n_slots + n_eval > cap:
            cap = max(2 * cap, n_slots + n_eval)
            b2 = torch.empty(cap, dtype=torch.int32, device=dev)
            v2 = torch.full((cap * 512,), float("nan"), dtype=torch.float32, device=dev)
            b2[:n_slots] = bricks[:n_slots]
            v2[:n_slots * 512] = values[:n_slots * 512]
            bricks, values = b2, v2
        L.surf_band_assign(_p(new_eval), n_eval, n_slots, _p(table), _p(bricks), _p(need), st)
        if n_eval:
            evaluate(bricks[n_slots:n_slots + n_eval], values[n_slots * 512:(n_slots + n_eval) * 512])
        n_slots += n_eval
        st = _stream()
        L.surf_band_clear(_p(new_cell), n_cell, _p(mark), st)
        L.surf_band_grow(_p(values), _p(table), _p(is_cell), _p(new_cell), n_cell, n, iso, _p(mark), st)
        if passes == 0:
            seeded = n_cell
        else:
            grown += n_cell
        passes += 1
    nbc, _ = band_dims(n)
    stats = {"bricks_screened": nbc ** 3, "bricks_seeded": seeded, "bricks_grown": grown, "bricks_evaluated": n_slots,
             "growth_iterations": passes, "band_points": n_slots * 512}
    return Band(n, table, is_cell, bricks[:n_slots], values[:n_slots * 512], stats)


def marching_cubes_band(band, isovalue=0.0, observed_only=False):
    """marching_cubes on a Band: (vertices (nv, 3) float64, triangles (nt, 3) int32) device tensors in lattice-index units, the
    arrays marching_cubes returns on the dense lattice (same order) for every surface component that has a cell brick.
    Two host syncs size the outputs (number of flagged points, then vertex / triangle totals).
    observed_only (fused bands: band.shape is the lattice, NaN = unobserved or not allocated): surf_band_classify_observed - the
    rule of marching_cubes(observed_only=True), every allocated brick meshed - and the same drop of unreferenced vertices."""
    L = _lib.lib()
    dev = band.values.device
    n, ns = band.resolution, band.n_slots
    iso = ctypes.c_double(float(isovalue))
    empty = torch.zeros(0, 3, dtype=torch.float64, device=dev), torch.zeros(0, 3, dtype=torch.int32, device=dev)
    if ns == 0:
        return empty
    flags = torch.empty(ns * 512, dtype=torch.uint8, device=dev)
    if observed_only:
        if band.shape is None or max(band.shape) != n:
            raise ValueError("marching_cubes_band: observed_only needs band.shape with max(shape) == resolution")
        nx, ny, nz = (int(v) for v in band.shape)
        L.surf_band_classify_observed(_p(band.values), _p(band.table), _p(band.bricks), ns, nx, ny, nz, iso, _p(flags), _stream())
    else:
        L.surf_band_classify(_p(band.values), _p(band.table), _p(band.is_cell), _p(band.bricks), ns, n, iso, _p(flags), _stream())
    pos = compact(flags)
    m = int(pos.shape[0])
    if m == 0:
        return empty
    keys = torch.empty(m, dtype=torch.int64, device=dev)
    L.surf_band_keys(_p(pos), m, _p(band.bricks), n, _p(keys), _stream())
    keys = torch.sort(keys).values                       # dense order: ascending lattice keys
    L.surf_band_rank(_p(keys), m, _p(band.table), n, _p(pos), _stream())
    ws = torch.empty(L.surf_mc_workspace_ints(m), dtype=torch.int32, device=dev)
    totals = torch.empty(2, dtype=torch.int32, device=dev)
    L.surf_mc_count(_p(flags), _p(pos), m, _p(ws), _p(totals), _stream())
    n_v, n_t = (int(v) for v in totals.tolist())
    vertices = torch.empty(n_v, 3, dtype=torch.float64, device=dev)
    triangles = torch.empty(n_t, 3, dtype=torch.int32, device=dev)
    vbase = torch.empty(ns * 512, dtype=torch.int32, device=dev)
    L.surf_band_emit(_p(band.values), _p(band.table), n, iso, _p(flags), _p(keys), _p(pos), m, _p(ws), _p(vbase), _p(vertices),
                     _p(triangles), _stream())
    if observed_only:
        return clean_update_faces(vertices, triangles, torch.ones(n_t, dtype=torch.uint8, device=dev))
    return vertices, triangles


# ------------------------------------------------------------------------------------------------
# sparse 3D U-Net pieces (reg_network.py)
# ------------------------------------------------------------------------------------------------

SUBM, DOWN, UP = 0, 1, 2


def table_from_coords(coords, D):
    table = torch.full((D, D, D), -1, dtype=torch.int32, device=coords.device)
    _lib.lib().surf_table_from_coords(_p(coords), coords.shape[0], int(D), _p(table), _stream())
    return table


# SURF_DOWN_DILATE / SURF_DOWN_FLOOR; "pad0" is the dilate kernel on coordinates stored + 1 with a fixed site range (below)
DOWN_RULES = {"dilate": 0, "floor": 1, "pad0": 0}
# The rule a conf without `reg_network.down_rule` gets (round 5): the reference pins torchsparse 2.1.0 (requirements.txt:205) and
# passes no padding (reg_network.py:9-13); that version's strided map is the spconv-style one = "pad0".
DEFAULT_DOWN_RULE = "pad0"
_pad0_ranges = {}


def down_sites(coords, D, rule=DEFAULT_DOWN_RULE, q_max=None):
    """Output sites of a k3/s2 sparse conv on the (D//2+1)^3 lattice: (coords2 (M,3) int32, table2, D2).
    rule: "dilate" (torchsparse's spdownsample for kernel != stride) or "floor" (unique(floor(c/2))): SURVEY App. C.
    "pad0" (the default): the spconv-style map with no padding (window 2q + {0,1,2}^3).  With every level's coordinates
    STORED + 1 (SparseCostRegNet.forward) that window is the centred one of the stored coordinates - 2 (q + 1) + {-1,0,1} =
    (2q + {0,1,2}) + 1 - so the same kernels serve; what differs is which even sites are outputs: all stored q in
    [1, q_max] with an input in the window (q_max = the true output lattice size (D_true - 3) // 2 + 1), instead of the even
    sites inside the inputs' bounding box."""
    _chk(coords, torch.int32, "coords")
    dev = coords.device
    D2 = D // 2 + 1
    if coords.shape[0] == 0:
        return (torch.empty(0, 3, dtype=torch.int32, device=dev), torch.full((D2, D2, D2), -1, dtype=torch.int32, device=dev), D2)
    if rule == "pad0":
        assert q_max is not None and q_max + 1 <= D2, (q_max, D2)
        key = (int(q_max), dev)
        if key not in _pad0_ranges:                                 # even sites 2 .. 2 q_max of the stored fine lattice
            _pad0_ranges[key] = torch.tensor([2, 2, 2, 2 * q_max, 2 * q_max, 2 * q_max], dtype=torch.int32, device=dev)
        bbox = _pad0_ranges[key]
    else:
        bbox = torch.empty(6, dtype=torch.int32, device=dev)          # stays on the device: no host round trip
        _lib.lib().surf_coords_bbox(_p(coords), coords.shape[0], _p(bbox), _stream())
    marks = torch.zeros(D2 * D2 * D2, dtype=torch.uint8, device=dev)
    _lib.lib().surf_mark_down_sites(_p(coords), coords.shape[0], int(D), _p(bbox), _p(marks), DOWN_RULES[rule], _stream())
    keys = compact(marks)
    c2 = torch.empty(keys.shape[0], 3, dtype=torch.int32, device=dev)
    t2 = torch.full((D2, D2, D2), -1, dtype=torch.int32, device=dev)
    if keys.shape[0] == 0:          # degenerate tiny lattices: no even site inside the inputs' bounding box
        return c2, t2, D2
    _lib.lib().surf_sites_from_keys(_p(keys), keys.shape[0], D2, _p(c2), _p(t2), _stream())
    return c2, t2, D2


def spconv_pack_weights(weight, thin=False):
    """(27, Cin, Cout) fp32 device kernel -> split bf16 operand image of surf_spconv_mfma, or None when the channel pair
    has no matrix-core kernel.  Pairs with Cin or Cout < 16 (the finest lattices) are only packed with thin=True: their
    matrix-core form pays under the bf16 training policy alone (one product per offset; csrc/spconv_mfma.hip)."""
    _chk(weight, torch.float32, "weight")
    cin, cout = int(weight.shape[1]), int(weight.shape[2])
    if min(cin, cout) < 16 and not thin:
        return None
    nbytes = _lib.lib().surf_spconv_packed_bytes(cin, cout)
    if nbytes == 0:
        return None
    packed = torch.empty(nbytes, dtype=torch.uint8, device=weight.device)
    _lib.lib().surf_spconv_pack_weights(_p(weight), cin, cout, _p(packed), _stream())
    return packed


def spconv(x, in_table, out_coords, mode, weight, bn_scale=None, bn_shift=None, skip=None, packed=None, bf16=False):
    """One sparse conv + BN(eval) + ReLU (+ skip).  x (n_in, Cin); weight (27, Cin, Cout); returns (n_out, Cout).
    packed (spconv_pack_weights(weight)): run the matrix-core kernel instead of the per-voxel one; bf16 (with packed): operands
    rounded to bf16, one product per k-step (the training policy train_precision = bf16; never used by inference)."""
    _chk(x, torch.float32, "x")
    _chk(in_table, torch.int32, "in_table")
    _chk(out_coords, torch.int32, "out_coords")
    _chk(weight, torch.float32, "weight")
    cin, cout = int(weight.shape[1]), int(weight.shape[2])
    assert x.shape[1] == cin and weight.shape[0] == 27
    out = torch.empty(out_coords.shape[0], cout, dtype=torch.float32, device=x.device)
    if out_coords.shape[0] == 0:
        return out
    if x.shape[0] == 0:             # no input rows: every lookup misses, the output is relu(bn_shift) (+ skip)
        x = torch.zeros(1, cin, dtype=torch.float32, device=x.device)
    if packed is not None:
        _chk(packed, torch.uint8, "packed weights")
        assert packed.numel() == _lib.lib().surf_spconv_packed_bytes(cin, cout)
        _lib.lib().surf_spconv_mfma(_p(x), cin, _p(in_table), int(in_table.shape[0]), _p(out_coords), out_coords.shape[0],
                                    int(mode), _p(packed), cout, _p(bn_scale), _p(bn_shift), _p(skip), _p(out), int(bool(bf16)),
                                    _stream())
        return out
    if bf16 and bf16_rows and cin == 16 and cout == 8 and bn_scale is None and skip is None and (mode == SUBM or bf16_rows_all_modes):
        # the bf16 training policy: gather from the rows' bf16 shadow (attached by bn_train_relu / bn_relu_backward, or made here)
        r16 = getattr(x, "_rows16", None)
        if r16 is None:
            r16 = rows_to_bf16(x)
        _lib.lib().surf_spconv_rows16(_p(r16), cin, _p(in_table), int(in_table.shape[0]), _p(out_coords), out_coords.shape[0],
                                      int(mode), _p(weight), cout, _p(out), _stream())
        return out
    _lib.lib().surf_spconv(_p(x), cin, _p(in_table), int(in_table.shape[0]), _p(out_coords), out_coords.shape[0], int(mode),
                           _p(weight), cout, _p(bn_scale), _p(bn_shift), _p(skip), _p(out), _stream())
    return out


count_pairs = False     # bench.py (set_count_pairs): count the (site, offset) pairs of every sparse-conv backward during its warm-up steps
_pair_counts = {}


def set_count_pairs(on):
    """Switch the pair counting of spconv_backward on / off.  The counts are cached per (mode, lattice, rows in, rows out) for
    ONE scene: switching it on forgets what an earlier scene left (two scenes whose sizes coincide must not share a count)."""
    global count_pairs
    if on:
        _pair_counts.clear()
    count_pairs = bool(on)


def dgrad_weights(weight, mode, use_mfma=True, thin=False):
    """Kernel of the input-gradient convolution of a sparse convolution with `weight` (27, Cin, Cout): slices transposed
    (27, Cout, Cin), offsets mirrored for the submanifold mode; + its split-bf16 operand image for surf_spconv_mfma (None when
    use_mfma is off or a channel count is below 16)."""
    wt = weight.transpose(1, 2).contiguous()
    if mode == SUBM:
        wt = wt.flip(0).contiguous()
    return wt, (spconv_pack_weights(wt, thin) if use_mfma else None)


wgrad_up_from_coarse = True     # False: the transposed layers' weight gradient walks the fine sites (the form until round 5; A/B)


def spconv_backward(x, in_table, in_coords, out_table, out_coords, mode, weight, dy, use_mfma=True, dgrad=None, on_side=False):
    """Backward of y = spconv(x, in_table, out_coords, mode, weight) (no BN / ReLU / skip).  Returns (dx (n_in, Cin),
    dW (27, Cin, Cout)).  dx is a sparse convolution of dy over the OUTPUT lattice (`out_table` indexes out_coords):
    submanifold with mirrored offsets, down <-> up, kernel slices transposed.
    use_mfma: the wide layers' input gradient on the matrix cores like their forward (surf_spconv_mfma, bf16x3: both channel
    counts >= 16; the per-voxel kernel sat at 0.02-0.18 of HBM there, round 3); False: every layer on the fp32 per-voxel kernel
    (SparseCostRegNet.use_mfma).  dgrad: a cached dgrad_weights(weight, mode, use_mfma) (SparseCostRegNet keeps one per block
    and parameter version).  on_side: the weight gradient is launched on `side` (SideStream) - the caller calls side.join()
    before it reads dW."""
    _chk(dy, torch.float32, "dy")
    cin, cout = int(weight.shape[1]), int(weight.shape[2])
    wt, wt_packed = dgrad if dgrad is not None else dgrad_weights(weight, mode, use_mfma)
    pairs = 0
    key = (int(mode), int(in_table.shape[0]), int(x.shape[0]), int(out_coords.shape[0]))
    if count_pairs and key not in _pair_counts and out_coords.shape[0] > 0 and x.shape[0] > 0:
        # bench only, OUTSIDE its timed region (warm-up steps; the lattices of the bench scene are the same every step): the
        # number of (output site, offset) pairs that exist = the forward convolution of an all-ones 8-channel input with a
        # constant kernel (1/8), summed; a device scalar
        ones = torch.ones(x.shape[0], 8, dtype=torch.float32, device=x.device)
        _pair_counts[key] = spconv(ones, in_table, out_coords, mode,
                                   torch.full((27, 8, 8), 0.125, dtype=torch.float32, device=x.device))[:, 0].sum()
    if kernel_events is not None:
        pairs = _pair_counts.get(key, 0)

    def dgrad_():
        with _timed(f"spconv_dgrad<{cout},{cin}>", {"pairs": pairs, "sites": int(in_coords.shape[0])}):
            return spconv(dy, out_table, in_coords, {SUBM: SUBM, DOWN: UP, UP: DOWN}[mode], wt, packed=wt_packed,
                          bf16=colgram_precision == 1)

    if out_coords.shape[0] == 0 or x.shape[0] == 0:
        return dgrad_(), small_zeros(weight.shape, weight.device)
    # the weight gradient of a TRANSPOSED layer is computed from the coarse side (round 5): fine site c takes from coarse site q
    # through offset o when c = 2 q + o, which is the stride-2 DOWN relation with the lattices' roles swapped - so
    # dW[k][ci][co] = sum_q x[q][ci] dy[fine(2 q + o_k)][co] is the DOWN-mode weight gradient of (input = dy on the fine lattice,
    # output sites = the coarse ones, upstream = x), transposed.  Walking the FINE sites instead, seven of eight (site, offset)
    # references are ruled out by parity and only found absent after the lookup: 8 x the sites for the same sum.
    swap = mode == UP and wgrad_up_from_coarse
    if swap:
        wx, wtab, wcoords, wmode, wdy, wci, wco = dy, out_table, in_coords, DOWN, x, cout, cin
    else:
        wx, wtab, wcoords, wmode, wdy, wci, wco = x, in_table, out_coords, mode, dy, cin, cout
    dW = small_zeros((27, wci, wco), weight.device)       # the kernels accumulate into it

    def wgrad():
        with _timed(f"spconv_wgrad<{cin},{cout}>", {"pairs": pairs, "sites": int(out_coords.shape[0])}):
            if use_mfma and _lib.lib().surf_spconv_wgrad_mfma_supported(wci, wco):
                # round 5: the channel pairs for which the matrix-core form wins (spconv_wgrad_mfma.hip), fp32-equivalent
                _lib.lib().surf_spconv_wgrad_mfma(_p(wx), wci, _p(wtab), int(wtab.shape[0]), _p(wcoords), wcoords.shape[0],
                                                  int(wmode), _p(wdy), wco, _p(dW), _stream())
            else:
                _lib.lib().surf_spconv_wgrad(_p(wx), wci, _p(wtab), int(wtab.shape[0]), _p(wcoords), wcoords.shape[0],
                                             int(wmode), _p(wdy), wco, _p(dW), _stream())

    if on_side:     # a leaf of the sweep: on the side stream, forked BEFORE the input gradient is issued so that the two run
        with side.fork():       # side by side (the caller joins before it reads dW)
            wgrad()
        side.keep(wx, wtab, wcoords, wdy, dW, lane=0)
        dx = dgrad_()
    else:
        dx = dgrad_()
        wgrad()
    if swap:
        dW = dW.transpose(1, 2)
    return dx, dW


def bn_train_relu(x, bn, skip=None, saved=None, counters=None, shadow=False):
    """spnn.BatchNorm in train mode + ReLU (+ skip) on raw convolution outputs x (n, C): batch statistics, running
    statistics updated in place like torch (reg_network.py:14-15,28-29).  bn: the block's nn.BatchNorm1d.
    saved: a dict that receives what bn_relu_backward needs (scale, shift, stats = mean | invstd).
    counters: a list that receives bn.num_batches_tracked INSTEAD of its increment - the caller bumps all of a network's
    counters with one torch._foreach_add_ (ten launches less per U-Net)."""
    _chk(x, torch.float32, "x")
    n, C = x.shape
    dev = x.device
    out = torch.empty_like(x)
    if n == 0:
        return out
    scale = torch.empty(C, dtype=torch.float32, device=dev)
    shift = torch.empty(C, dtype=torch.float32, device=dev)
    stats = torch.empty(2 * C, dtype=torch.float32, device=dev) if saved is not None else None
    ws = torch.empty(_lib.lib().surf_bn_workspace_bytes(C), dtype=torch.uint8, device=dev)
    momentum = 0.1 if bn.momentum is None else float(bn.momentum)
    track = bn.track_running_stats and bn.running_mean is not None
    _lib.lib().surf_bn_train_affine(_p(x), n, C, _p(bn.weight.detach()), _p(bn.bias.detach()), float(bn.eps), momentum,
                                    _p(bn.running_mean if track else None), _p(bn.running_var if track else None),
                                    _p(scale), _p(shift), _p(stats), _p(ws), _stream())
    if track:
        if counters is not None:
            counters.append(bn.num_batches_tracked)
        else:
            bn.num_batches_tracked += 1
    if saved is not None:
        saved.update(scale=scale, shift=shift, stats=stats)
    out16 = torch.empty(n, C, dtype=torch.int16, device=dev) if shadow else None     # shadow: the rows' bf16 copy (ops.bf16_rows)
    _lib.lib().surf_bn_relu_apply16(_p(x), n, C, _p(scale), _p(shift), _p(skip), _p(out), _p(out16), _stream())
    if shadow:
        out._rows16 = out16
    return out


def bn_relu_backward(x, dy, scale, shift, stats, train=True, shadow=False):
    """Backward of bn_train_relu (train) / of the folded eval-mode BN + ReLU (train=False): x the raw convolution output
    (n, C), dy the gradient of the block output (which is also the skip's gradient), scale / shift the forward's affine,
    stats = mean | invstd (2C).  Returns (dx (n, C), dgamma (C), dbeta (C))."""
    _chk(x, torch.float32, "x")
    _chk(dy, torch.float32, "dy")
    n, C = x.shape
    dev = x.device
    dx = torch.empty_like(x)
    if n == 0:
        return dx, small_zeros((C,), dev), small_zeros((C,), dev)
    dgb = torch.empty(2, C, dtype=torch.float32, device=dev)       # bn_bwd_finalize_kernel writes (not accumulates) both rows
    dgamma, dbeta = dgb[0], dgb[1]
    ws = torch.empty(_lib.lib().surf_bn_workspace_bytes(C), dtype=torch.uint8, device=dev)
    mean, invstd = stats[:C], stats[C:]
    dx16 = torch.empty(n, C, dtype=torch.int16, device=dev) if shadow else None
    _lib.lib().surf_bn_relu_backward16(_p(x), _p(dy), n, C, _p(scale), _p(shift), _p(mean), _p(invstd), int(bool(train)),
                                       _p(ws), _p(dgamma), _p(dbeta), _p(dx), _p(dx16), _stream())
    if shadow:
        dx._rows16 = dx16
    return dx, dgamma, dbeta


def row_linear8(x, weight):
    _chk(x, torch.float32, "x")
    _chk(weight, torch.float32, "weight")
    assert x.shape[1] == 8 and tuple(weight.shape) == (8, 8)
    out = torch.empty_like(x)
    _lib.lib().surf_row_linear8(_p(x), _p(weight), x.shape[0], _p(out), _stream())
    return out


# ------------------------------------------------------------------------------------------------
# FPN pieces (feature_network.py)
# ------------------------------------------------------------------------------------------------


def conv3x3(x, w_packed, cout, stride=1, precision=0):
    """x (N,H,W,Cin) NHWC, w_packed [3][3][Cin][Cout] -> (N,H/stride,W/stride,Cout).  precision (layers with Cin >= 16, which run
    on the matrix cores): 0 = fp32-equivalent (exact bf16x3 split), 1 = operands rounded to bf16 (the bf16 training policy)."""
    _chk(x, torch.float32, "x")
    _chk(w_packed, torch.float32, "weight")
    N, H, W, cin = x.shape
    out = torch.empty(N, H // stride, W // stride, cout, dtype=torch.float32, device=x.device)
    _lib.lib().surf_conv3x3_p(_p(x), _p(w_packed), N, H, W, cin, cout, stride, _p(out), int(precision), _stream())
    return out


def deconv3x3_s2(x, w_packed, cout, precision=0):
    _chk(x, torch.float32, "x")
    _chk(w_packed, torch.float32, "weight")
    N, H, W, cin = x.shape
    out = torch.empty(N, 2 * H, 2 * W, cout, dtype=torch.float32, device=x.device)
    _lib.lib().surf_deconv3x3_s2_p(_p(x), _p(w_packed), N, H, W, cin, cout, _p(out), int(precision), _stream())
    return out


def conv3x3_wgrad(big, small, stride=1, precision=0):
    """out[ky][kx][cb][cs] = sum big[n][ys S + ky - 1][xs S + kx - 1][cb] small[n][ys][xs][cs]: the weight gradient of a 3x3
    convolution (big = input, small = d output) or of the stride-2 transposed one (big = d output, small = input)."""
    _chk(big, torch.float32, "big")
    _chk(small, torch.float32, "small")
    N, Hs, Ws, cs = small.shape
    cb = big.shape[3]
    assert tuple(big.shape[:3]) == (N, Hs * stride, Ws * stride)
    ws = torch.empty(_lib.lib().surf_conv3x3_wgrad_workspace_floats(N, Hs, Ws, cb, cs), dtype=torch.float32, device=big.device)
    out = torch.empty(3, 3, cb, cs, dtype=torch.float32, device=big.device)
    _lib.lib().surf_conv3x3_wgrad_p(_p(big), _p(small), N, Hs, Ws, cb, cs, int(stride), _p(ws), _p(out), int(precision), _stream())
    return out


def inorm_relu_backward(raw, dy, stats):
    """Backward of inorm_relu_ (the skip's gradient is dy itself): raw (N,H,W,C) the convolution output before the in-place
    normalisation, stats (N,C,2) = mean | rstd.  One call for all views (surf_inorm_relu_backward: blockIdx.y = view; until
    round 5 a Python loop of surf_bn_relu_backward per view with sliced statistics: ~600 small launches per training step)."""
    _chk(raw, torch.float32, "raw")
    _chk(dy, torch.float32, "dy")
    _chk(stats, torch.float32, "stats")
    N, H, W, C = raw.shape
    assert tuple(dy.shape) == tuple(raw.shape) and tuple(stats.shape) == (N, C, 2)
    if C not in (8, 16, 32, 64):
        raise ValueError(f"inorm_relu_backward: C = {C} channels; instantiated for C in (8, 16, 32, 64)")
    dx = torch.empty_like(raw)
    ws = torch.empty(_lib.lib().surf_inorm_backward_workspace_bytes(N, C), dtype=torch.uint8, device=raw.device)
    _lib.lib().surf_inorm_relu_backward(_p(raw), _p(dy), N, H * W, C, _p(stats), _p(ws), _p(dx), _stream())
    return dx


def inorm_relu_(x, skip=None, want_stats=False, in_place=True):
    """x = relu(instance_norm(x)) (+ skip); x (N,H,W,C) NHWC.  in_place (default): x is overwritten and returned; False: x is
    left as it is (a recording forward keeps it as the raw convolution output) and a new tensor is returned."""
    _chk(x, torch.float32, "x")
    N, H, W, C = x.shape
    if C not in (4, 8, 16, 32, 64):
        raise ValueError(f"inorm_relu_: C = {C} channels; the FPN kernels are instantiated for C in (4, 8, 16, 32, 64) "
                         "(feature_network d_base = 8; include/surf_hip.h: surf_inorm_relu)")
    ws = torch.empty(_lib.lib().surf_inorm_workspace_doubles(N, H, W, C), dtype=torch.float64, device=x.device)
    stats = torch.empty(N, C, 2, dtype=torch.float32, device=x.device)
    out = x if in_place else torch.empty_like(x)
    _lib.lib().surf_inorm_relu_out(_p(x), N, H, W, C, _p(skip), _p(ws), _p(stats), _p(out), _stream())
    return (out, stats) if want_stats else out


# ------------------------------------------------------------------------------------------------
# small fused helpers of the training step (csrc/train_small.hip)
# ------------------------------------------------------------------------------------------------

def occupied_any(pts, volumes):
    """lookup_volume(pts, mask_volumes, 'nearest').any(-1) (implicit_surface.py:175) in one launch: (n,) bool."""
    _chk(pts, torch.float32, "pts")
    assert pts.dim() == 2 and pts.shape[1] == 3
    out = torch.empty(pts.shape[0], dtype=torch.bool, device=pts.device)
    if pts.shape[0] == 0:
        return out
    _lib.lib().surf_occupied_any(_p(pts), pts.shape[0], volumes._tp, volumes._dp, volumes.n, _p(out), _stream())
    return out


_l1_counters = {}


def _l1_mask(mask, ref):
    """(tensor or None, mask_kind of surf_masked_l1) for a mask given as a float / bool tensor or the string "target>0"."""
    if isinstance(mask, str):
        assert mask == "target>0"
        return None, 2
    assert mask.numel() == ref.numel() and mask.device == ref.device
    if mask.dtype == torch.bool or mask.dtype == torch.uint8:
        return mask.contiguous(), 1
    return _chk(mask.float().contiguous(), torch.float32, "mask"), 0


def masked_l1(pred, target, mask):
    """sum(|pred - target| mask) / (sum(mask) + 1e-8) as ONE launch (loss.py:71-93; fp64 sums in a fixed order).  mask: a float /
    bool tensor of pred's size, or "target>0".  Returns out2 (2,) fp32: [0] the loss, [1] 1 / (sum(mask) + 1e-8)."""
    _chk(pred, torch.float32, "pred")
    _chk(target, torch.float32, "target")
    assert pred.numel() == target.numel() and pred.numel() > 0
    dev = pred.device
    m, kind = _l1_mask(mask, pred)
    key = (dev.index, torch.cuda.current_stream().cuda_stream)
    if key not in _l1_counters:        # one self-resetting arrival counter per stream
        _l1_counters[key] = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = torch.empty(_lib.lib().surf_masked_l1_workspace_bytes(), dtype=torch.uint8, device=dev)
    out2 = torch.empty(2, dtype=torch.float32, device=dev)
    _lib.lib().surf_masked_l1(_p(pred), _p(target), _p(m), kind, pred.numel(), _p(ws), _p(_l1_counters[key]), _p(out2), _stream())
    return out2


def masked_l1_backward(pred, target, mask, out2, upstream):
    """d (upstream * masked_l1) / d pred; upstream: a 0-d fp32 device tensor."""
    m, kind = _l1_mask(mask, pred)
    up = _chk(upstream.reshape(1).float().contiguous(), torch.float32, "upstream")
    g = torch.empty_like(pred)
    _lib.lib().surf_masked_l1_backward(_p(pred), _p(target), _p(m), kind, pred.numel(), _p(out2), _p(up), _p(g), _stream())
    return g


def weight_norm_backward(vs, gs, dWs):
    """Backward of W_l = g_l v_l / |v_l|_row (sdf_network.py:88-89) for a list of layers in ONE launch: ([dv_l], [dg_l]),
    dg_l shaped like g_l."""
    n = len(vs)
    assert n == len(gs) == len(dWs) and n >= 1
    for v, g, dW in zip(vs, gs, dWs):
        _chk(v, torch.float32, "weight_v")
        _chk(g, torch.float32, "weight_g")
        _chk(dW, torch.float32, "dW")
        assert v.dim() == 2 and dW.shape == v.shape and g.numel() == v.shape[0]
    dvs = [torch.empty_like(v) for v in vs]
    dgs = [torch.empty_like(g) for g in gs]
    rows = (ctypes.c_int * n)(*[int(v.shape[0]) for v in vs])
    cols = (ctypes.c_int * n)(*[int(v.shape[1]) for v in vs])
    _lib.lib().surf_weight_norm_backward(n, _ptr_array(vs), _ptr_array(gs), _ptr_array(dWs), rows, cols, _ptr_array(dvs),
                                         _ptr_array(dgs), _stream())
    return dvs, dgs


# ------------------------------------------------------------------------------------------------
# point-cloud clean-up (point_knn.hip): k nearest neighbours within a cloud, outlier statistic, normals
# ------------------------------------------------------------------------------------------------

POINTS_KNN_MAX_K = 32                # SURF_POINTS_KNN_MAX_K of include/surf_hip.h
POINTS_KNN_MAX_CELLS = 1 << 26       # SURF_POINTS_KNN_MAX_CELLS
POINTS_STAT_SLOTS = 1024             # SURF_POINTS_STAT_SLOTS


def _chk_knn(k, max_dist, what):
    """The argument checks of the surf_points_knn* entry points, as ValueError before the call."""
    if int(k) != k or not 1 <= k <= POINTS_KNN_MAX_K:
        raise ValueError(f"{what}: k must be an integer in [1, {POINTS_KNN_MAX_K}], got {k}")
    md = float(np.float32(max_dist))
    md2 = float(np.float32(md) * np.float32(md))
    if not (md > 0 and np.isfinite(md) and md2 > 0 and np.isfinite(md2)):
        raise ValueError(f"{what}: max_dist must be finite and > 0 (and so must its fp32 square), got {max_dist}")
    return int(k), md


class PointKnnTable:
    """The dense cell table over one cloud (n, 3) fp32 that surf_points_knn / _reduce search: nearest_dist_capped's pattern (a key
    kernel, torch's sort, bincount and cumsum), the cell grown by 1.25 until the table has at most POINTS_KNN_MAX_CELLS cells.
    Points with a non-finite coordinate sort behind the table.  cell: the cell size to start from (tests; the results do not depend
    on it), default: about four cells per point by the box's volume, at least max_dist / 16 (an isolated point walks at most 17
    shells).  Two host syncs (the box of the finite points)."""

    def __init__(self, points, max_dist, cell=None):
        _chk(points, torch.float32, "points")
        if points.dim() != 2 or points.shape[1] != 3:
            raise ValueError(f"points: expected (n, 3), got {tuple(points.shape)}")
        n = points.shape[0]
        if n > 2 ** 31 - 1:
            raise ValueError(f"points: {n} points exceed int32 indexing")
        if n == 0:
            raise ValueError("PointKnnTable: empty cloud")
        dev = points.device
        finite = points[torch.isfinite(points).all(1)]
        if finite.shape[0]:
            lo, hi = finite.amin(0).double().tolist(), finite.amax(0).double().tolist()
        else:
            lo, hi = [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]
        del finite
        ext = [b - a for a, b in zip(lo, hi)]
        if cell is not None:
            cell = float(cell)
        if cell is None or cell > 0:                  # (a given cell that is NaN or <= 0 has no table: the check below raises)
            cell, dims = _table_cell_dims(ext, n, float(max_dist) / 16.0, POINTS_KNN_MAX_CELLS, cell)
        if not (cell > 0 and np.isfinite(cell)):
            raise ValueError(f"PointKnnTable: cell must be finite and > 0, got {cell}")
        ncell = dims[0] * dims[1] * dims[2]
        keys = torch.empty(n, dtype=torch.int64, device=dev)
        _lib.lib().surf_points_knn_keys(_p(points), n, lo[0], lo[1], lo[2], cell, dims[0], dims[1], dims[2], _p(keys), _stream())
        self.cstart, self.spts, order = _cell_table(points, keys, ncell, tail=True)
        self.points = points
        self.sidx = order.to(torch.int32)
        self.lo, self.cell, self.dims, self.n = lo, cell, dims, n
        self.cells_per_point = ncell / n

    def _grid(self):
        return (self.lo[0], self.lo[1], self.lo[2], self.cell, self.dims[0], self.dims[1], self.dims[2])


def _knn_table(points, max_dist, cell):
    return points if isinstance(points, PointKnnTable) else PointKnnTable(points, max_dist, cell)


def points_knn(points, k, max_dist, cell=None):
    """The neighbour lists of rule 1 (include/surf_hip.h): (index (n, k) int32 padded with -1, d2 (n, k) fp32 padded with +inf, count
    (n,) int32) of a cloud (n, 3) fp32 on the device, or of a PointKnnTable over it."""
    k, max_dist = _chk_knn(k, max_dist, "points_knn")
    if not isinstance(points, PointKnnTable) and points.shape[0] == 0:
        _chk(points, torch.float32, "points")
        dev = points.device
        return (torch.empty(0, k, dtype=torch.int32, device=dev), torch.empty(0, k, dtype=torch.float32, device=dev),
                torch.empty(0, dtype=torch.int32, device=dev))
    T = _knn_table(points, max_dist, cell)
    dev = T.spts.device
    index = torch.empty(T.n, k, dtype=torch.int32, device=dev)
    d2 = torch.empty(T.n, k, dtype=torch.float32, device=dev)
    count = torch.empty(T.n, dtype=torch.int32, device=dev)
    _lib.lib().surf_points_knn(_p(T.spts), _p(T.sidx), _p(T.cstart), T.n, *T._grid(), k, max_dist, _p(index), _p(d2), _p(count),
                               _stream())
    return index, d2, count


def points_knn_reduce(points, k, max_dist, normals=False, view=None, centres=None, cell=None):
    """The same search without the lists: (stat (n,) fp32, count (n,) int32, normal (n, 3) fp32 or None) by rules 2 and 5.
    view (n,) int32 and centres (n_views, 3) fp64 (device tensors, both or neither) orient the normals."""
    k, max_dist = _chk_knn(k, max_dist, "points_knn_reduce")
    if (view is None) != (centres is None):
        raise ValueError("points_knn_reduce: view and centres are given together")
    if view is not None and not normals:
        raise ValueError("points_knn_reduce: view / centres orient normals: pass normals=True")
    if not isinstance(points, PointKnnTable) and points.shape[0] == 0:
        _chk(points, torch.float32, "points")
        dev = points.device
        return (torch.empty(0, dtype=torch.float32, device=dev), torch.empty(0, dtype=torch.int32, device=dev),
                torch.empty(0, 3, dtype=torch.float32, device=dev) if normals else None)
    T = _knn_table(points, max_dist, cell)
    dev = T.spts.device
    n_views = 0
    if view is not None:
        _chk(view, torch.int32, "view")
        _chk(centres, torch.float64, "centres")
        if view.shape != (T.n,):
            raise ValueError(f"view: expected ({T.n},), got {tuple(view.shape)}")
        if centres.dim() != 2 or centres.shape[1] != 3 or centres.shape[0] < 1:
            raise ValueError(f"centres: expected (n_views >= 1, 3), got {tuple(centres.shape)}")
        n_views = centres.shape[0]
    stat = torch.empty(T.n, dtype=torch.float32, device=dev)
    count = torch.empty(T.n, dtype=torch.int32, device=dev)
    normal = torch.empty(T.n, 3, dtype=torch.float32, device=dev) if normals else None
    _lib.lib().surf_points_knn_reduce(_p(T.points), _p(T.spts), _p(T.sidx), _p(T.cstart), T.n, *T._grid(), k, max_dist, _p(view),
                                      _p(centres), n_views, _p(stat), _p(count), _p(normal), _stream())
    return stat, count, normal


def points_stat_sums(stat):
    """(3,) float64 device tensor [number, sum, sum of squares] of the finite values of stat (n,) fp32 (rule 3): fixed-slot partial
    sums added in slot order, the same bits on every run."""
    _chk(stat, torch.float32, "stat")
    if stat.dim() != 1:
        raise ValueError(f"stat: expected (n,), got {tuple(stat.shape)}")
    part = torch.empty(POINTS_STAT_SLOTS * 3, dtype=torch.float64, device=stat.device)
    out = torch.empty(3, dtype=torch.float64, device=stat.device)
    _lib.lib().surf_points_stat_sums(_p(stat), stat.shape[0], _p(part), _p(out), _stream())
    return out


# ------------------------------------------------------------------------------------------------
# point-set surface (point_surface.hip): a signed distance on the lattice bricks near an oriented cloud
# ------------------------------------------------------------------------------------------------

CLOUD_MAX_RING = 4                   # SURF_CLOUD_MAX_RING of include/surf_hip.h
CLOUD_INDEX_BITS = 31                # a composite key is (brick key << 31) | caller index


def cloud_ring(reach):
    """ring = ceil(reach / 8) of rule 2 (include/surf_hip.h, above surf_cloud_brick_keys), as ValueError where the entry points
    would return a status."""
    reach = float(reach)
    if not (reach > 0 and reach < 1e9):
        raise ValueError(f"point surface: reach must be finite and > 0 lattice steps, got {reach}")
    ring = int(np.ceil(reach / 8.0))
    if ring > CLOUD_MAX_RING:
        raise ValueError(f"point surface: the support reaches across {ring} bricks, at most {CLOUD_MAX_RING} are supported "
                         f"(a radius just under {8 * CLOUD_MAX_RING} voxels)")
    return ring


def _cloud_frame(axes, lo, voxel):
    nx, ny, nz = _chk_fuse_axes(axes)
    lo = [float(v) for v in np.asarray(lo, np.float64).reshape(3)]
    return (lo[0], lo[1], lo[2], float(voxel), nx, ny, nz)


def cloud_sort(points, normals, colors, axes, lo, voxel, reach):
    """Rules 1-3: (sorted_keys (m,) int64, sorted_points (m, 3), sorted_normals (m, 3), sorted_colors (m, 3) uint8 or None) of the
    points of the cloud that take part, in ascending composite-key order.  points, normals (n, 3) fp32, colors (n, 3) uint8 or
    None, device tensors.  One host read (m)."""
    _chk(points, torch.float32, "points")
    _chk(normals, torch.float32, "normals")
    if points.dim() != 2 or points.shape[1] != 3 or normals.shape != points.shape:
        raise ValueError(f"point surface: points and normals (n, 3), got {tuple(points.shape)} and {tuple(normals.shape)}")
    if colors is not None:
        _chk(colors, torch.uint8, "colors")
        if colors.shape != points.shape:
            raise ValueError(f"point surface: colors (n, 3) uint8, got {tuple(colors.shape)}")
    n = int(points.shape[0])
    if n > 2 ** 31 - 1:
        raise ValueError(f"points: {n} points exceed int32 indexing")
    ring = cloud_ring(reach)
    frame = _cloud_frame(axes, lo, voxel)
    keys = torch.empty(n, dtype=torch.int64, device=points.device)
    _lib.lib().surf_cloud_brick_keys(_p(points), _p(normals), n, *frame, float(reach), _p(keys), _stream())
    tail = 1
    for a in frame[4:]:
        tail *= (a + 7) // 8 + 2 * ring
    skeys = torch.sort(keys)[0]
    m = int((skeys < (tail << CLOUD_INDEX_BITS)).sum()) if n else 0
    skeys = skeys[:m].contiguous()
    order = skeys & ((1 << CLOUD_INDEX_BITS) - 1)
    return (skeys, points[order].contiguous(), normals[order].contiguous(),
            None if colors is None else colors[order].contiguous())


def cloud_mark_bricks(mark, sorted_points, axes, lo, voxel, reach):
    """Rule 6: mark (nbp^3 bytes, see fuse_brick_dims) gets a 1 at every brick a point of sorted_points (m, 3) allocates."""
    _chk(mark, torch.uint8, "mark")
    _chk(sorted_points, torch.float32, "sorted_points")
    frame = _cloud_frame(axes, lo, voxel)
    if mark.numel() != fuse_brick_dims(frame[4:])[1] ** 3:
        raise ValueError("cloud_mark_bricks: mark holds one byte per brick of the table")
    cloud_ring(reach)
    _lib.lib().surf_cloud_mark_bricks(_p(sorted_points), int(sorted_points.shape[0]), *frame, float(reach), _p(mark), _stream())


def cloud_field_bricks(sorted_cloud, bricks, axes, lo, voxel, reach, radius, min_points, staged=False):
    """Rules 3-5 at every node of the listed bricks: (tsdf, weight (n_bricks * 512,), color (n_bricks * 512, 3) or None[, staged
    (n_bricks,) int32: the candidates every brick ran through]).  sorted_cloud: cloud_sort's tuple."""
    skeys, spts, snrm, scol = sorted_cloud
    _chk(skeys, torch.int64, "sorted_keys")
    _chk(spts, torch.float32, "sorted_points")
    _chk(snrm, torch.float32, "sorted_normals")
    _chk(bricks, torch.int32, "bricks")
    m, nb = int(skeys.shape[0]), int(bricks.shape[0])
    if spts.shape != (m, 3) or snrm.shape != (m, 3) or (scol is not None and (scol.dtype != torch.uint8 or scol.shape != (m, 3))):
        raise ValueError("cloud_field_bricks: sorted keys (m,), points and normals (m, 3) fp32, colours (m, 3) uint8")
    if int(min_points) != min_points or min_points < 1:
        raise ValueError(f"cloud_field_bricks: min_points must be an integer >= 1, got {min_points}")
    if nb * 512 >= 2 ** 31:
        raise ValueError("point surface: 2^31 / 512 allocated bricks or more")
    cloud_ring(reach)
    frame = _cloud_frame(axes, lo, voxel)
    dev = bricks.device
    tsdf = torch.empty(nb * 512, dtype=torch.float32, device=dev)
    weight = torch.empty(nb * 512, dtype=torch.float32, device=dev)
    color = None if scol is None else torch.empty(nb * 512, 3, dtype=torch.float32, device=dev)
    count = torch.empty(nb, dtype=torch.int32, device=dev) if staged else None
    _lib.lib().surf_cloud_field_bricks(_p(skeys), _p(spts), _p(snrm), _p(scol), m, _p(bricks), nb, _p(axes[0]), _p(axes[1]),
                                       _p(axes[2]), *frame[4:], *frame[:4], float(reach), ctypes.c_float(float(radius)),
                                       int(min_points), _p(tsdf), _p(weight), _p(color), _p(count), _stream())
    return (tsdf, weight, color) + ((count,) if staged else ())
