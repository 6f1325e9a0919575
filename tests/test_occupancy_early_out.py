"""The occupancy test of ray_setup_kernel and occupied_any_kernel walks the index tables smallest first and leaves the loop at a
lane's first hit.  The result is an OR over the levels, so neither the order the caller lists them in nor whether they are nested
may show: both kernels against the nearest lookup of every level done in torch on the very points the ray set-up returns."""
import pytest
import torch

pytestmark = pytest.mark.gpu

R, N_SAMPLES = 37, [64, 32, 16, 16]          # 37 rays: ten workgroups of four wavefronts, the last one with a clamped ray


def _tables(kind, dev):
    """Index tables, coarse -> fine.  'pyramid': 8^3 .. 64^3 that are NOT nested - the coarsest level holds the half space x < 0
    thinned at random, the finest a random 6 % of the whole cube, the two between 3 % each, so some places are occupied at the
    finest level only and others at the coarsest only."""
    g = torch.Generator().manual_seed(11)
    dims = [8] if kind == "single" else [8, 16, 32, 64]
    out = []
    for s, D in enumerate(dims):
        if kind == "empty":
            keep = torch.zeros(D, D, D, dtype=torch.bool)
        elif kind == "full":
            keep = torch.ones(D, D, D, dtype=torch.bool)
        elif s == 0:
            keep = torch.rand(D, D, D, generator=g) < 0.6
            if kind != "single":
                keep[D // 2:] = False
        else:
            keep = torch.rand(D, D, D, generator=g) < (0.06 if s == 3 else 0.03)
        table = torch.full((D, D, D), -1, dtype=torch.int32)
        table[keep] = torch.arange(int(keep.sum()), dtype=torch.int32)
        out.append(table.to(dev))
    return out


def _nearest(pts, table):
    """lookup_volume(pts, mask, 'nearest') of one level: round-half-even of the unnormalised coordinate, zeros outside."""
    D = table.shape[0]
    gi = torch.round(((pts + 1.0) * D - 1.0) / 2.0).long()
    ok = ((gi >= 0) & (gi < D)).all(dim=-1)
    gi = gi.clamp(0, D - 1)
    return ok & (table[gi[:, 0], gi[:, 1], gi[:, 2]] >= 0)


@pytest.mark.parametrize("kind,fine_first", [("pyramid", True), ("pyramid", False), ("single", True), ("empty", True),
                                             ("full", False)])
def test_vmask_and_occupied_any_are_the_or_over_levels(kind, fine_first):
    from surf_amd import ops, synthetic
    dev = torch.device("cuda:0")
    tabs = _tables(kind, dev)
    if fine_first:
        tabs = tabs[::-1]
    sv = ops.SparseVolumes([torch.zeros(max(int((t >= 0).sum()), 1), 8, device=dev) for t in tabs], tabs)
    H, W = 32, 48
    intrs, c2ws, near_fars = synthetic.ring_cameras(3, H, W)
    rays_o, rays_d = synthetic.pixel_rays(intrs[0], c2ws[0], H, W, 1, dev)
    pick = torch.linspace(0, rays_o.shape[0] - 1, R).long().to(dev)
    rays_o, rays_d = rays_o[pick].contiguous(), rays_d[pick].contiguous()
    near = near_fars[0, 0].reshape(1, 1).repeat(R, 1).to(dev)
    far = near_fars[0, 1].reshape(1, 1).repeat(R, 1).to(dev)
    D = 16
    ax = torch.arange(D, dtype=torch.float32, device=dev) * (2.0 / (D - 1)) - 1.0
    mvol = -20.0 * (torch.sqrt(ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2) - 0.5).abs()
    st = ops.ray_setup(rays_o, rays_d, near, far, mvol.contiguous(), sv, N_SAMPLES, [1.0, 0.4, 0.1, 0.01], 256)
    pts = st["pts"]
    assert pts.shape == (R * sum(N_SAMPLES), 3) and sum(N_SAMPLES) == 128
    per_level = [_nearest(pts, t) for t in tabs]
    want = torch.stack(per_level).any(dim=0)
    assert torch.equal(st["vmask"].bool(), want)
    assert torch.equal(ops.occupied_any(pts, sv), want)
    if kind == "pyramid":                          # the construction holds what it promises, on these very sample points
        coarse, fine = (per_level[-1], per_level[0]) if fine_first else (per_level[0], per_level[-1])
        others = torch.stack(per_level[1:-1]).any(dim=0)
        assert bool((fine & ~coarse & ~others).any()) and bool((coarse & ~fine & ~others).any())
        assert bool(want.any()) and not bool(want.all())
    elif kind == "empty":
        assert not bool(want.any())
    elif kind == "full":                           # the rays do cross the cube
        assert bool(want.any())
