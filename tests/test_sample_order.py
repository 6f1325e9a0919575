"""Order of the active-sample list (surf_compact_blocked, render.sample_block): the set flags of an (R, S) ray-major array in
the traversal order (ray // G, s // B, ray % G, s % B), so that a 32-sample tile of the SDF / blend kernels holds B consecutive
samples of G neighbouring rays.  The entries stay flat ray-major indices: a permutation of surf_compact's list.  Neither MLP
kernel looks across samples (tests/test_sdf_dealing.py, tests/test_blend_dealing.py), so a render may not change by a bit."""
import pytest
import torch

RAYS = (1, 7, 8, 9, 33, 100)                    # R < G, ragged last ray blocks, whole blocks
SAMPLES = (4, 128)
DENSITIES = (0.0, 0.5, 0.93, 1.0)


def blocks_of(S):
    return ((1, S), (4, 4), (8, 4), (32, 1), (4, S))


def blocked_order(R, S, G, B, device="cpu"):
    """The flat ray-major indices r * S + s of an (R, S) array in the order (r // G, s // B, r % G, s % B); the last ray block
    holds R % G rays when G does not divide R."""
    assert S % B == 0
    flat = torch.arange(R * S, dtype=torch.int64, device=device).view(R, S)
    full = R // G
    head = flat[:full * G].view(full, G, S // B, B).permute(0, 2, 1, 3).reshape(-1)
    tail = flat[full * G:].view(R - full * G, S // B, B).permute(1, 0, 2).reshape(-1)
    return torch.cat([head, tail])


def test_blocked_order_is_a_permutation_and_ray_major_is_the_identity():
    for R, S, G, B in [(R, S, G, B) for R in RAYS for S in SAMPLES for G, B in blocks_of(S)] + [(33_000, 128, 8, 4)]:
        order = blocked_order(R, S, G, B)
        assert torch.equal(order.sort().values, torch.arange(R * S)), (R, S, G, B)
        if (G, B) == (1, S):
            assert torch.equal(order, torch.arange(R * S)), (R, S)
    # by hand: 3 rays of 4 samples, blocks of 2 rays x 2 samples; the last block is one ray
    assert blocked_order(3, 4, 2, 2).tolist() == [0, 1, 4, 5, 2, 3, 6, 7, 8, 9, 10, 11]


def _flags(n, density, seed, device, offset=0):
    """n flag bytes (set ones are 1, 2 or 255) at `offset` bytes into their allocation"""
    g = torch.Generator().manual_seed(seed)
    on = torch.rand(n, generator=g) < density
    val = torch.tensor([1, 2, 255], dtype=torch.uint8)[torch.randint(0, 3, (n,), generator=g)]
    buf = torch.zeros(n + offset, dtype=torch.uint8, device=device)
    buf[offset:] = torch.where(on, val, torch.zeros_like(val)).to(device)
    return buf[offset:]


def _check(flags, R, S, G, B):
    from surf_amd import ops
    idx, count = ops.compact_counted(flags, block=(S, G, B))
    order = blocked_order(R, S, G, B, flags.device)
    want = order[flags[order] != 0].to(torch.int32)
    assert idx.dtype == torch.int32 and idx.shape == (R * S,) and count.shape == (1,)
    assert int(count) == want.numel(), (R, S, G, B, int(count), want.numel())
    assert torch.equal(idx[:want.numel()], want), (R, S, G, B)
    return idx, count


@pytest.mark.gpu
@pytest.mark.parametrize("S", SAMPLES)
def test_blocked_compaction_equals_the_restatement(S):
    from surf_amd import ops
    d = torch.device("cuda:0")
    for R in RAYS:
        for k, density in enumerate(DENSITIES):
            for offset in (0, 1):                                # a whole allocation; one that is not 16-byte aligned
                flags = _flags(R * S, density, 100 * R + k, d, offset)
                assert (flags.data_ptr() % 16 != 0) == bool(offset)
                for G, B in blocks_of(S):
                    idx, count = _check(flags, R, S, G, B)
                    if (G, B) == (1, S):                         # ray-major: surf_compact's list, entry for entry
                        idx0, count0 = ops.compact_counted(flags)
                        n = int(count0)
                        assert int(count) == n and torch.equal(idx[:n], idx0[:n])


@pytest.mark.gpu
def test_blocked_compaction_across_the_scan_chunk():
    """33,000 x 128 flags = 1,032 blocks of 4,096: the single-block scan of the block counts takes a second chunk of 1,024."""
    R, S = 33_000, 128
    flags = _flags(R * S, 0.5, 9, torch.device("cuda:0"))
    assert (R * S + 4095) // 4096 > 1024
    _check(flags, R, S, 8, 4)


@pytest.mark.gpu
def test_blocked_compaction_refuses_other_blocks():
    from surf_amd import ops
    flags = torch.ones(7 * 4, dtype=torch.uint8, device="cuda:0")
    for block in ((4, 4, 8), (4, 3, 4), (4, 4, 3), (4, 0, 4), (4, 4, 0)):      # S % B != 0; G, B no powers of two
        with pytest.raises(RuntimeError):
            ops.compact_counted(flags, block=block)
    with pytest.raises(ValueError):
        ops.compact_counted(flags, block=(8, 4, 4))                            # 28 flags are no rays of 8 samples


N_SAMPLES = [16, 8, 8, 8]                       # 40 per ray: a multiple of 8 (and of 4)


@pytest.fixture(scope="module")
def render_scene_inputs():
    """__graft_entry__.smoke's render on the dealing tests' 44^3 pyramid with 5 views; 96 rays in pixel order."""
    from surf_amd import ops, synthetic
    dev = torch.device("cuda:0")
    H, W, nv = 32, 48, 5
    intrs, c2ws, near_fars = synthetic.ring_cameras(nv, H, W)
    imgs = synthetic.procedural_images(nv, H, W, 0, dev)
    feats = synthetic.feature_pyramid(nv, H, W, 0, dev)
    vols, tabs, mvol = synthetic.sphere_pyramid(44, dev)
    rays_o, rays_d = synthetic.pixel_rays(intrs[0], c2ws[0], H, W, 4, dev)
    return dict(dev=dev, vols=vols, tabs=tabs, mvol=mvol, feats=feats, imgs=imgs, intrs=intrs.to(dev), c2ws=c2ws.to(dev),
                rays_o=rays_o.contiguous(), rays_d=rays_d.contiguous(), near=float(near_fars[0, 0]), far=float(near_fars[0, 1]))


def _render_both_orders(p, precision, rays_o, rays_d, near, far):
    """(outputs in the default block order, outputs in ray-major order, number of active samples)"""
    from bench import model_conf
    from surf_amd import ops
    from surf_amd.implicit_surface import SAMPLE_BLOCK, ImplicitSurface
    dev = p["dev"]
    R = rays_o.shape[0]
    near_t = torch.full((R, 1), near, device=dev)
    far_t = torch.full((R, 1), far, device=dev)
    outs = []
    for block in (None, [1, 0]):
        conf = model_conf(N_SAMPLES, sdf_precision=precision, blend_precision=precision)
        if block is not None:
            conf["render"]["sample_block"] = block
        torch.manual_seed(0)
        model = ImplicitSurface(conf).to(dev)
        assert model.sample_block == (SAMPLE_BLOCK if block is None else (1, 0))
        with torch.no_grad():
            model.deviation_network.variance.fill_(0.45)
        scene = model.scene(p["mvol"], p["vols"][::-1], p["tabs"][::-1], None, p["feats"], p["imgs"], p["intrs"], p["c2ws"])
        outs.append(model.render_scene(rays_o, rays_d, near_t, far_t, scene, 1.0, per_sample=True))
    st = ops.ray_setup(rays_o, rays_d, near_t, far_t, p["mvol"], scene.sv, N_SAMPLES, [1.0, 0.4, 0.1, 0.01], 256)
    return outs[0], outs[1], int(st["vmask"].sum())


def _assert_same(a, b):
    assert set(a) == set(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["bf16x3", "f16x2"])
def test_render_does_not_depend_on_the_sample_order(render_scene_inputs, precision):
    from surf_amd.implicit_surface import SAMPLE_BLOCK
    p = render_scene_inputs
    G, B = SAMPLE_BLOCK
    assert B > 0 and sum(N_SAMPLES) % B == 0, "the default order must be a blocked one that this render takes"
    ro, rd = p["rays_o"], p["rays_d"]
    R = ro.shape[0]
    # every ray; a ray count that is no multiple of G (and one ray: fewer rays than a block)
    for n_rays in (R, R - 3, 1):
        assert n_rays == 1 or n_rays > G and (n_rays % G != 0) == (n_rays != R)
        a, b, n_act = _render_both_orders(p, precision, ro[:n_rays].contiguous(), rd[:n_rays].contiguous(), p["near"], p["far"])
        assert n_act > 32 * (n_rays > 1)
        _assert_same(a, b)
    # rays that look away from the scene: no active sample at all
    a, b, n_act = _render_both_orders(p, precision, ro, (-rd).contiguous(), p["near"], p["far"])
    assert n_act == 0
    _assert_same(a, b)
    # the centre ray between depths 3 and 5 (it leaves the volume's cube at 3.5) beside two that look away: fewer than 32
    mid = R // 2 + 6
    ro3 = ro[mid:mid + 3].contiguous()
    rd3 = torch.stack([rd[mid], -rd[mid + 1], -rd[mid + 2]]).contiguous()
    a, b, n_act = _render_both_orders(p, precision, ro3, rd3, 3.0, 5.0)
    assert 0 < n_act < 32, n_act
    _assert_same(a, b)
