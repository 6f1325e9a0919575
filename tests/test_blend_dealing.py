"""blend_split_kernel deals its 32-sample tiles on demand: a wavefront's first tile is its own index, every further run of tiles
comes from one counter in the caller's scratch buffer, which the entry point zeroes on the launch stream before every launch.
A sample is one column of the tile and nothing crosses columns, so which wavefront evaluates a tile, and in which launch, may
not change a bit of its colour or its view count."""
import pytest
import torch

pytestmark = pytest.mark.gpu

# 70,001 samples = 2,188 tiles: more than the 2,048 resident wavefronts, so the counter hands out the rest (runs of one tile)
SIZES = (1, 31, 32, 33, 70_001)
TOL = {"bf16x3": 1.0, "f16x2": 4.0}            # x 3e-6 absolute against the fp32 kernel: test_blend_split_view_counts' bound


@pytest.fixture(scope="module")
def inputs(scene, weights, golden_fpn):
    from surf_amd import ops
    d = torch.device("cuda:0")
    feats = [ops.pack_texel4(golden_fpn[f"out{i}"].to(d).contiguous()) for i in range(4)][::-1]      # fine -> coarse
    imgs = ops.pack_texel4(scene["imgs"].to(d).contiguous())
    g = torch.Generator().manual_seed(77)
    pts = ((torch.rand(2_100_017, 3, generator=g) * 2 - 1) * 0.7).to(d).contiguous()
    out = {"pts": pts, "w32": ops.blend_pack_weights(weights, d)}
    nv0 = int(scene["intrs"].shape[0])
    for ns in (2, 4, 6):
        sel = [i % nv0 for i in range(ns + 1)]                       # views beyond the scene's five repeat earlier ones
        out[ns] = ([f[sel].contiguous() for f in feats], imgs[sel].contiguous(), ops.Cameras(scene["intrs"][sel], scene["c2ws"][sel]))
    for prec in TOL:
        out[prec] = ops.blend_pack_weights(weights, d, precision=prec)
    return out


def _close(a, b, atol):
    err = float((a - b).abs().max())
    assert err <= atol, err


@pytest.mark.parametrize("ns", [2, 4, 6])
@pytest.mark.parametrize("precision", ["bf16x3", "f16x2"])
def test_dealt_tiles_equal_tile_by_tile_evaluation(inputs, precision, ns):
    from surf_amd import ops
    feats, imgs, cams = inputs[ns]
    w = inputs[precision]
    for n in SIZES:
        p = inputs["pts"][:n].contiguous()
        a, na = ops.blend(p, feats, imgs, cams, w)
        b, nb = ops.blend(p, feats, imgs, cams, w)                   # back to back on one stream: the counter starts at zero again
        assert torch.equal(a, b) and torch.equal(na, nb), n
        parts = [ops.blend(p[i:i + 32].contiguous(), feats, imgs, cams, w) for i in range(0, n, 32)]   # one tile per launch
        assert torch.equal(a, torch.cat([c for c, _ in parts])) and torch.equal(na, torch.cat([k for _, k in parts])), n
        c32, n32 = ops.blend(p, feats, imgs, cams, inputs["w32"])
        _close(a, c32, 3e-6 * TOL[precision])
        assert torch.equal(na, n32) and (n < 1000 or int(na.max()) == ns)
    # the count read from device memory, below the capacity of the index list: the tiles past it are nobody's
    n, used = SIZES[-1], 50_003
    idx = torch.arange(n, dtype=torch.int32, device=p.device)
    count = torch.tensor([used], dtype=torch.int32, device=p.device)
    for _ in range(2):
        c, k = ops.blend(p, feats, imgs, cams, w, active_idx=idx, active_count=count)
        assert torch.equal(c[:used], a[:used]) and torch.equal(k[:used], na[:used])
        assert bool((c[used:] == 0).all()) and bool((k[used:] == 0).all())


@pytest.mark.parametrize("precision", ["bf16x3", "f16x2"])
def test_run_lengths_do_not_show(inputs, precision):
    """2,100,017 samples = 65,626 tiles, 32 per resident wavefront: runs of four tiles.  Its halves (32,813 tiles each) are dealt
    in runs of two, pieces of 262,144 samples in single tiles: the same bits every way."""
    from surf_amd import ops
    feats, imgs, cams = inputs[4]
    w, p = inputs[precision], inputs["pts"]
    n = p.shape[0]
    assert (n + 31) // 32 >= 32 * 2048 and 16 * 2048 <= (n // 2 + 31) // 32 < 32 * 2048
    a, na = ops.blend(p, feats, imgs, cams, w)
    b, nb = ops.blend(p, feats, imgs, cams, w)
    assert torch.equal(a, b) and torch.equal(na, nb)
    for step in (n // 2 + 1, 262_144):
        parts = [ops.blend(p[i:i + step].contiguous(), feats, imgs, cams, w) for i in range(0, n, step)]
        assert torch.equal(a, torch.cat([c for c, _ in parts])) and torch.equal(na, torch.cat([k for _, k in parts])), step
    c32, n32 = ops.blend(p, feats, imgs, cams, inputs["w32"])
    _close(a, c32, 3e-6 * TOL[precision])
    assert torch.equal(na, n32)
