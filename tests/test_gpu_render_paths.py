"""Depth renderer on the MI355X (csrc/render.hip) on the paths that tests/test_gpu_render.py leaves unexecuted, against the
float64 restatement of tests/render_ref.py and under that file's bars:

  * a splat block whose staging buffer fills and is scanned in the MIDDLE of its point range (more than CAP - SUB = 768 staged
    points of its per_split): the (best, index) state carried over the scans, the compaction over several fills, and the
    lowest-index rule between two fills of one block.  render_ref.split_plan restates the host's split rule, and every test
    that claims this path asserts on its plan before it renders;
  * render_bwd_kernel<false>, the backward that reads the argmax map from global memory (w > 128), at w = 192 and w = 256;
  * rho other than 24: the culling radius, the backward's pixel window and the rho == 0 branch.

Run with `pytest -m gpu`."""
import pytest
import torch

import render_ref as RR
from scream_amd import _lib, ops
from scream_amd.render import RegistrationRender, rotation_matrix, view_eulers

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILL = 768  # CAP - SUB of render_splat_kernel: a block scans in mid-range once more than this many points are staged


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_native_lib():
    assert torch.cuda.is_available(), "pytest -m gpu needs the MI355X"
    _lib.load()


def clouds(n, m, seed, lo=-0.9, hi=0.9):
    g = torch.Generator().manual_seed(seed)
    src = torch.rand(n, 3, generator=g) * (hi - lo) + lo
    tgt = torch.rand(m, 3, generator=g) * (hi - lo) + lo
    return src.to(DEV), tgt.to(DEV)


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return (torch.linalg.norm(a - b) / max(torch.linalg.norm(b).item(), 1e-300)).item()


def i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def check_float64(what, src, tgt, w, rho, eulers, imgs, amax, up, grad):
    """One pair's images [V,2,w,w], argmax and source gradient [n,3] (of sum(imgs * up)) under the three bars of
    tests/test_gpu_render.py.  At least half of the pixels must be compared for the argmax; a one-point source cloud cannot
    give that on its own channel (its image is 0 outside one spot, test_images_against_float64 exempts it too), so there the
    target channel alone has to."""
    ref64, amax64, _, gap64 = RR.render(src.double(), tgt.double(), rho, w, eulers, dtype=torch.float64, top2=True)
    ref32 = RR.render(src, tgt, rho, w, eulers, dtype=torch.float32)[0]
    err = (imgs.double() - ref64).abs().max().item()
    err32 = (ref32.double() - ref64).abs().max().item()
    sure = gap64 > 1e-5
    share = sure[:, 1].float().mean().item() if src.shape[0] == 1 else sure.float().mean().item()
    wrong = (amax.long()[sure] != amax64[sure]).sum().item()
    g64 = RR.backward(src.double(), tgt.double(), up, amax, rho, w, eulers, dtype=torch.float64)
    g32 = RR.backward(src, tgt, up, amax, rho, w, eulers, dtype=torch.float32)
    r, r32 = rel(grad, g64), rel(g32, g64)
    print("%s: image err %.3g (fp32 restatement %.3g, bar %.3g); argmax compared on %.3f of the pixels, %d differ; "
          "gradient rel %.3g (fp32 restatement %.3g, bar %.3g)"
          % (what, err, err32, max(2 * err32, 1e-6), share, wrong, r, r32, max(2 * r32, 1e-5)))
    assert err <= max(2 * err32, 1e-6), (err, err32)
    assert share >= 0.5, share
    assert wrong == 0
    assert g64.abs().max() > 0
    assert r <= max(2 * r32, 1e-5), (r, r32)


def check_batch_against_single_calls(what, lens, w, view, plan, float64_pairs, seed):
    """len(lens) pairs in one call, packed with gaps of garbage rows: the call's split plan is `plan` with per_split >= 2000
    (several fills per block), every pair's own call has per_split <= 768 (none), and both give the same bits."""
    eulers = view_eulers(view)
    V, B, rho = len(eulers), len(lens), 24
    max_s, max_t = max(n for n, _ in lens), max(m for _, m in lens)
    got_plan = RR.split_plan(w, B, V, max(max_s, max_t))
    single_plans = [RR.split_plan(w, 1, V, max(n, m)) for n, m in lens]
    print("%s: split_plan %s; single-pair per_split %d .. %d"
          % (what, got_plan, min(p for _, p in single_plans), max(p for _, p in single_plans)))
    assert got_plan == plan and got_plan[1] >= 2000
    assert all(p <= FILL for _, p in single_plans)
    pairs = [clouds(n, m, seed=seed + i) for i, (n, m) in enumerate(lens)]
    rot = torch.stack([rotation_matrix(e) for e in eulers]).to(DEV)
    s_parts, t_parts, s_row0, t_row0, r_s, r_t = [], [], [], [], 0, 0
    for (s, t) in pairs:  # padding rows hold garbage the kernels must not read
        s_row0.append(r_s)
        t_row0.append(r_t)
        s_parts += [s, torch.full((37, 3), 1e30, device=DEV)]
        t_parts += [t, torch.full((11, 3), -1e30, device=DEV)]
        r_s += s.shape[0] + 37
        r_t += t.shape[0] + 11
    S, T = torch.cat(s_parts), torch.cat(t_parts)
    s_len, t_len = [n for n, _ in lens], [m for _, m in lens]
    ws = ops.render_workspace(B, V, w, S.shape[0], DEV)
    imgs, amax = ops.render_depth(S, i32(s_row0), i32(s_len), T, i32(t_row0), i32(t_len), max_s, max_t, rot, w, rho, ws)
    up = torch.randn(imgs.shape, device=DEV, generator=torch.Generator(DEV).manual_seed(seed))
    dS = ops.render_depth_bwd(up, amax, S, i32(s_row0), i32(s_len), max_s, rot, w, rho, ws)
    differ = []
    for i, (s, t) in enumerate(pairs):
        meta = i32([0, s.shape[0], 0, t.shape[0]])
        ws1 = ops.render_workspace(1, V, w, s.shape[0], DEV)
        im1, am1 = ops.render_depth(s, meta[0:1], meta[1:2], t, meta[2:3], meta[3:4], s.shape[0], t.shape[0], rot, w, rho, ws1)
        d1 = ops.render_depth_bwd(up[i:i + 1].contiguous(), am1, s, meta[0:1], meta[1:2], s.shape[0], rot, w, rho, ws1)
        same = (torch.equal(imgs[i], im1[0]), torch.equal(amax[i], am1[0]), torch.equal(dS[s_row0[i]:s_row0[i] + s.shape[0]], d1))
        if not all(same):
            differ.append((i, lens[i]) + same)
    pad = torch.ones(S.shape[0], dtype=torch.bool, device=DEV)
    for r, n in zip(s_row0, s_len):
        pad[r:r + n] = False
    print("%s: pairs whose (images, argmax, dsrc) differ from their own call: %s; padding rows with a gradient: %d"
          % (what, differ, (dS[pad] != 0).any(dim=1).sum().item()))
    assert not differ
    assert torch.equal(dS[pad], torch.zeros_like(dS[pad]))
    for i in float64_pairs:
        s, t = pairs[i]
        check_float64("%s pair %d %s" % (what, i, lens[i]), s, t, w, rho, eulers, imgs[i], amax[i], up[i],
                      dS[s_row0[i]:s_row0[i] + s.shape[0]])


# a B = 16 step of the training workload's geometry: ranges that end on and next to the boundaries of a 2500-point split, at
# and next to the sizes of the staging buffer (768, 1024), a one-point cloud on either side
LENS_W64 = [(7500, 7500), (7499, 2501), (1, 2500), (769, 1024), (1025, 769), (2500, 7499), (2501, 1), (5000, 5000), (5001, 2499),
            (4999, 5001), (768, 257), (256, 3000), (257, 768), (3333, 6000), (6100, 1300), (900, 4097)]
LENS_W256 = [(3000, 2500), (2999, 3000), (1, 1500), (769, 1024), (1025, 769), (1500, 2999), (1501, 1), (2000, 2000), (768, 257),
             (256, 1333), (257, 768), (1333, 2047), (2500, 900), (900, 2500), (2047, 256), (3000, 3000)]


def test_several_fills_per_block_equal_single_pair_calls_bitwise_w64():
    # 4 tiles * 192 images = 768 blocks -> 3 splits of 2500 points: at w = 64 nearly every point is staged, three scans a block
    check_batch_against_single_calls("w64 x 6 views", LENS_W64, 64, "muti", (3, 2500), float64_pairs=(0, 2, 5), seed=100)


def test_unsplit_ranges_and_global_map_backward_equal_single_pair_calls_bitwise_w256():
    # 64 tiles * 32 images = 2048 blocks: no split at all, a block walks a whole cloud; the backward is render_bwd_kernel<false>
    check_batch_against_single_calls("w256 x 1 view", LENS_W256, 256, "single", (1, 3000), float64_pairs=(0, 1), seed=200)


@pytest.mark.parametrize("n,m,w,view,rho", [(1500, 1500, 192, "single", 24), (3000, 3000, 64, "muti", 0),
                                            (3000, 3000, 64, "muti", 4), (3000, 3000, 64, "muti", 96)])
def test_single_pairs_against_float64_and_repeatable(n, m, w, view, rho):
    src, tgt = clouds(n, m, seed=300 + w + rho)
    gen = RegistrationRender(rho, w, view=view)
    print("w %d rho %d: split_plan %s" % (w, rho, RR.split_plan(w, 1, len(gen.eulers), max(n, m))))
    s = src.clone().requires_grad_(True)
    out = gen(s, tgt)
    up = torch.randn(out.shape, device=DEV, generator=torch.Generator(DEV).manual_seed(3))
    g1 = torch.autograd.grad((out * up).sum(), s)[0]
    out2 = gen(s, tgt)
    g2 = torch.autograd.grad((out2 * up).sum(), s)[0]
    rot = gen.view_matrices(DEV)
    meta = i32([0, n, 0, m])
    imgs, amax = ops.render_depth(src, meta[0:1], meta[1:2], tgt, meta[2:3], meta[3:4], n, m, rot, w, rho)
    print("repeat: images %s, gradient %s; ops.render_depth images %s"
          % (torch.equal(out, out2), torch.equal(g1, g2), torch.equal(imgs[0], out.detach())))
    assert torch.equal(out, out2) and torch.equal(g1, g2) and torch.equal(imgs[0], out.detach())
    if rho == 0:
        # g = 1 everywhere: a view's image is the largest pv of its side at every pixel, and the side that holds the pair's
        # nearest point (pv = 1 - 0 / span) is (1 - 0.5) / 0.5 = 1 exactly
        x64 = torch.cat([src, tgt]).double()
        sides = [int(torch.argmin(x64 @ rot[v, 2].double()).item() >= n) for v in range(rot.shape[0])]
        ones = [torch.equal(out[v, side], torch.ones_like(out[v, side])) for v, side in enumerate(sides)]
        print("rho 0: side of the nearest point per view %s, its image all 1.0: %s" % (sides, ones))
        assert not torch.isnan(out).any() and all(ones)
    check_float64("(%d, %d) w %d rho %d" % (n, m, w, rho), src, tgt, w, rho, gen.eulers, out.detach(), amax[0], up, g1)


def test_duplicates_in_a_later_fill_of_the_same_block_lose_to_the_lowest_index():
    w, n = 256, 4000
    splits, per_split = RR.split_plan(w, 1, 6, n)
    # clouds in +-0.7: at +-0.9 a central tile of w = 256 stages 750 of its first 1280 points, short of a mid-range scan
    src, tgt = clouds(n, 3000, seed=9, lo=-0.7, hi=0.7)
    # rows 0..49: over the central tiles of the identity view and nearest in it, so that they win pixels there
    g = torch.Generator().manual_seed(10)
    src[:50, :2] = (torch.rand(50, 2, generator=g) * 0.5 - 0.25).to(DEV)
    src[:50, 2] = (torch.rand(50, generator=g) * 0.1 - 0.7).to(DEV)
    first, last = 1280, 3900
    src[first:first + 50] = src[:50]  # the sixth staging step of the block of rows 0..1333
    src[last:last + 50] = src[:50]    # another block: the merge of the 64-bit keys
    # tile (3, 3) of the identity view holds the pixel centres -0.246 .. -0.004 in x and in y.  Every point within
    # sqrt(0.38) of that square is staged (0.38 * cexp = -157.9 > CULL_T), and a block scans once more than 768 are:
    # that many among rows 0..1279 put the scan between rows 0..49 and their copies at rows 1280..1329.
    d = (torch.clamp(-0.246 - src[:first, :2].double(), min=0) + torch.clamp(src[:first, :2].double() + 0.004, min=0)) ** 2
    staged = int((d.sum(dim=1) <= 0.38).sum().item())
    print("split_plan %s; points of rows 0..%d staged by tile (3, 3) of view 0: %d" % ((splits, per_split), first - 1, staged))
    assert (splits, per_split) == (3, 1334) and first + 50 <= per_split and last >= 2 * per_split
    assert first % 256 == 0 and staged > FILL
    gen = RegistrationRender(24, w)
    s = src.clone().requires_grad_(True)
    out = gen(s, tgt)
    up = torch.randn(out.shape, device=DEV, generator=torch.Generator(DEV).manual_seed(0))
    grad = torch.autograd.grad((out * up).sum(), s)[0]
    meta = i32([0, n, 0, 3000])
    amax = ops.render_depth(src, meta[0:1], meta[1:2], tgt, meta[2:3], meta[3:4], n, 3000, gen.view_matrices(DEV), w, 24)[1][0, :, 0]
    centre = amax[0, 96:160, 96:160]  # tiles (3..4, 3..4) of the identity view
    counts = [int(((amax >= a) & (amax < a + 50)).sum().item()) for a in (0, first, last)]
    print("pixels won by rows 0..49 / %d.. / %d..: %s; by rows 0..49 in the central tiles of view 0: %d; |grad| there %.3g / %.3g / %.3g"
          % (first, last, counts, int(((centre >= 0) & (centre < 50)).sum().item()), grad[:50].abs().sum().item(),
             grad[first:first + 50].abs().sum().item(), grad[last:last + 50].abs().sum().item()))
    assert counts[1] == 0 and counts[2] == 0
    assert counts[0] > 0 and ((centre >= 0) & (centre < 50)).any()
    assert torch.equal(grad[first:first + 50], torch.zeros(50, 3, device=DEV))
    assert torch.equal(grad[last:last + 50], torch.zeros(50, 3, device=DEV))
    assert grad[:50].abs().sum() > 0
