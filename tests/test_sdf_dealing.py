"""The gradient instantiation of sdf_mlp_split_kernel deals its rounds (4 tiles of 32 samples) on demand: a workgroup's first
round is its own index, every further one comes from one counter in front of the caller's scratch slots, which the entry point
zeroes on the launch stream before every launch; wavefront 0 hands the value to the other three through two LDS words.
A sample is one column of a tile and nothing crosses columns, tiles or wavefronts, so which workgroup evaluates a round, and
in which launch, may not change a bit of sdf or grad.

The grid is min(rounds, 256), so the counter is first asked for work beyond 256 rounds = 32,768 samples:
  1, 127, 128, 129   one or two rounds, dealing is never asked
  32,768             256 rounds: every workgroup asks once and is told there is nothing
  32,769             exactly one dealt round with one live sample (three of its wavefronts hold only padding)
  98,381             769 = 3 x 256 + 1 rounds, ragged last tile: some workgroups take three or more rounds (both LDS words)"""
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = (1, 127, 128, 129, 32_768, 32_769, 98_381)
N = SIZES[-1]


@pytest.fixture(scope="module")
def problem():
    """tests/test_hip_stress.py's problem (perturbed weights: the volume channels matter), unmasked, with its fp32 reference."""
    from bench import model_conf
    from surf_amd import ops, synthetic
    from surf_amd.implicit_surface import ImplicitSurface
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = ImplicitSurface(model_conf([64, 32, 16, 16])).to(dev)
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        for l in range(1, 7):
            lin = getattr(model.sdf_network, f"lin{l}")
            lin.weight_v[:, -28:] += (0.05 * torch.randn(lin.weight_v.shape[0], 28, generator=g)).to(dev)
    vols, tabs, mvol = synthetic.sphere_pyramid(44, dev)
    sv = ops.SparseVolumes(vols[::-1], tabs[::-1])
    pts = ((torch.rand(N, 3, generator=g) * 2 - 1) * 0.6).to(dev).contiguous()
    sd = {k: v for k, v in model.state_dict().items()}
    s_ref, g_ref = ops.sdf_mlp(pts, sv, ops.sdf_pack_weights(sd, dev, "sdf_network."))
    out = dict(dev=dev, sv=sv, pts=pts, s_ref=s_ref, g_ref=g_ref)
    for prec in ("bf16x3", "f16x2"):
        out[prec] = ops.sdf_pack_weights_split(sd, dev, "sdf_network.", prec)
    return out


def _pieces(p, w, n, step):
    from surf_amd import ops
    parts = [ops.sdf_mlp(p["pts"][i:min(i + step, n)].contiguous(), p["sv"], w) for i in range(0, n, step)]
    return torch.cat([s for s, _ in parts]), torch.cat([g for _, g in parts])


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("precision", ["bf16x3", "f16x2"])
def test_dealt_rounds_equal_round_by_round_evaluation(problem, precision, n):
    from surf_amd import ops
    p, w = problem, problem[precision]
    pts = p["pts"][:n].contiguous()
    s, g = ops.sdf_mlp(pts, p["sv"], w)
    s2, g2 = ops.sdf_mlp(pts, p["sv"], w)              # back to back on one stream: the counter starts at zero again
    assert torch.equal(s, s2) and torch.equal(g, g2)
    for step in (128, 32_768):                         # one round per launch / 256 rounds per launch: nothing is dealt
        sp, gp = _pieces(p, w, n, step)
        assert torch.equal(s, sp) and torch.equal(g, gp), step
    es = float((s - p["s_ref"][:n]).abs().max())
    eg = float((g - p["g_ref"][:n]).abs().max())
    assert es <= 1e-4 and eg <= 1e-3, (es, eg)         # test_hip_stress.py's bounds against the fp32 kernel


@pytest.mark.parametrize("precision", ["bf16x3", "f16x2"])
def test_device_side_count_below_capacity(problem, precision):
    """The `_dn` entry points: grid and scratch follow the capacity, the rounds follow the count read on the device."""
    from surf_amd import ops
    p, w = problem, problem[precision]
    dev = p["dev"]
    full_s, full_g = ops.sdf_mlp(p["pts"], p["sv"], w)
    idx = torch.arange(N, dtype=torch.int32, device=dev)
    ones = torch.ones(N, dtype=torch.uint8, device=dev)    # a mask makes ops.sdf_mlp fill the outputs: 100 / 0
    for used in (50_003, 200, 0):                          # 391 rounds; 2 rounds (fewer than workgroups); none
        count = torch.tensor([used], dtype=torch.int32, device=dev)
        for _ in range(2):
            s, g = ops.sdf_mlp(p["pts"], p["sv"], w, mask=ones, active_idx=idx, active_count=count)
            assert torch.equal(s[:used], full_s[:used]) and torch.equal(g[:used], full_g[:used]), used
            assert bool((s[used:] == 100.0).all()) and bool((g[used:] == 0.0).all()), used
