"""Yardstick of the training tests: seeded inputs, the float64 / fp32 CPU oracle's gradients under torch autograd, optionally
under the relu masks and L1 signs of ANOTHER path through the same network, and the rule every gradient tensor is held to.

Why masks: the FFN relu, the two relus of coor_mlp and the L1 loss are piecewise.  A hidden unit within rounding of zero is
switched differently by each fp32 path than by float64, and ONE such unit moves whole tensors by 1e-4 .. 5e-4 relative, two
orders of magnitude above fp32 rounding.  Given the masks and signs of the path under test, the oracle differentiates the same
smooth function as that path (relu(x) -> x * m, abs(x) -> x * s), and what is left between them is rounding.

The rule (`rule`): per parameter tensor, rel(g, g64m) <= max(2 * e32m, FLOOR), where g64m is the float64 oracle under the masks
of g's own forward pass and e32m the fp32 CPU oracle's error against g64m UNDER THE SAME MASKS.

Mask keys are the oracle's block applications, (state_dict prefix, "src" | "tgt"), plus ("coor_mlp.0.", "src") and
("coor_mlp.2.", "src"); "sign" holds the L1 signs [1,N,3].  One dict per pair of a batch."""
import numpy as np
import torch

from oracle import scream_ref as O
from scream_amd.synthetic import random_rotation

FLOOR = 5e-6  # the fixed floor of the "<= 2 x the fp32 path's error" rule
RATIO = 2


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return (torch.linalg.norm(a - b) / max(torch.linalg.norm(b).item(), 1e-300)).item()


def packed_rows(lens, rng, width, pad_value=0.0):
    """[sum(padded lens), width] with real rows random and padded tails `pad_value`."""
    parts = []
    for n in lens:
        p = (n + 127) // 128 * 128
        x = np.full((p, width), pad_value, dtype=np.float32)
        x[:n] = rng.standard_normal((n, width)).astype(np.float32)
        parts.append(x)
    return torch.from_numpy(np.concatenate(parts))


def make_pair(seed, n, m):
    """One seeded registration pair: src [1,n,3], tgt [1,m,3], rot [1,3,3], trans [1,3,1] with rot src + trans ~ tgt."""
    rng = np.random.default_rng(seed)
    tgt = rng.uniform(-0.6, 0.6, size=(m, 3)).astype(np.float32)
    R = random_rotation(rng, 30.0).astype(np.float32)
    t = rng.uniform(-0.1, 0.1, size=(3, 1)).astype(np.float32)
    base = tgt[rng.permutation(m)[:n]] if n <= m else np.concatenate([tgt, rng.uniform(-0.6, 0.6, size=(n - m, 3))])
    src = ((base - t.T) @ R + 0.005 * rng.standard_normal((n, 3))).astype(np.float32)  # R src + t ~ tgt
    return (torch.from_numpy(src)[None], torch.from_numpy(tgt)[None], torch.from_numpy(R)[None], torch.from_numpy(t)[None])


def terrain(seed, points):
    """One seeded OpenGF-like sample: dsm [1,N,3], dem_coarse [1,M,3], dem [1,N,3] (CPU, divided by 50)."""
    from scream_amd.evaluate_open_gf import SyntheticDEM
    dsm, coarse, dem, _ = SyntheticDEM(1, seed, points)[0]
    return dsm[None], coarse[None], dem[None]


# ------------------------------------------------------------------------------------- the oracle's gradients
def _leaves(sd, dtype):
    return {k: v.detach().clone().to(dtype).requires_grad_() for k, v in sd.items()}


def oracle_grads(sd, src, tgt, rot, trans, dtype, masks=None, record=None):
    """(loss, {name: gradient}) of PointTransformer + point_loss on one pair.  masks: the dict described above (relu masks and
    "sign"); record: a dict that receives this run's own masks and signs in that form."""
    sdx = _leaves(sd, dtype)
    c = lambda t: t.to(dtype)
    relu = None if masks is None else {k: v for k, v in masks.items() if k != "sign"}
    pred = O.point_transformer_forward(c(src), c(tgt), sdx, c(trans).permute(0, 2, 1), masks=relu, record_masks=record)
    if record is not None:
        record["sign"] = torch.sign(pred.detach() - O.registered(c(src), c(rot), c(trans)))
    loss = O.point_loss(pred, c(src), c(rot), c(trans), None if masks is None else masks["sign"])
    loss.backward()
    return loss.item(), {k: v.grad for k, v in sdx.items()}


def dem_oracle_grads(sd, dsm, coarse, dem, dtype, masks=None, record=None):
    """oracle_grads for DEMTransformer + its plain L1 loss on one sample."""
    sdx = _leaves(sd, dtype)
    relu = None if masks is None else {k: v for k, v in masks.items() if k != "sign"}
    pred = O.dem_transformer_forward(dsm.to(dtype), coarse.to(dtype), sdx, masks=relu, record_masks=record)
    if record is not None:
        record["sign"] = torch.sign(pred.detach() - dem.to(dtype))
    loss = O.dem_loss(pred, dem.to(dtype), None if masks is None else masks["sign"])
    loss.backward()
    return loss.item(), {k: v.grad for k, v in sdx.items()}


def masked_oracles(grads_fn, sd, samples, masks):
    """(g64m, g32m): the float64 and the fp32 oracle's gradients of the MEAN loss over `samples` (one tuple of grads_fn's data
    arguments each), every sample under its own dict of `masks`."""
    out = []
    for dtype in (torch.float64, torch.float32):
        per = [grads_fn(sd, *s, dtype, masks=m)[1] for s, m in zip(samples, masks)]
        out.append({k: sum(g[k] for g in per) / len(per) for k in sd})
    return out


# ------------------------------------------------------------------------------------- the rule
def rule(what, g, g64m, g32m, ratio=RATIO, floor=FLOOR):
    """The tensors that miss rel(g, g64m) <= max(ratio * rel(g32m, g64m), floor), as (name, error, e32m).  Prints the worst."""
    bad, worst = [], (0.0, None, 0.0, 0.0)
    assert set(g) == set(g64m) == set(g32m)
    for k in g64m:
        e, e32 = rel(g[k], g64m[k]), rel(g32m[k], g64m[k])
        bar = max(ratio * e32, floor)
        if e / bar > worst[0]:
            worst = (e / bar, k, e, e32)
        if not e <= bar:
            bad.append((k, e, e32))
    print("%s: worst tensor %s at %.3g of its bar (error %.3g, fp32 oracle under the same masks %.3g); largest error %.3g; "
          "largest error / fp32 oracle's %.3g; %d of %d over the bar"
          % (what, worst[1], worst[0], worst[2], worst[3], max(rel(g[k], g64m[k]) for k in g64m),
             max(rel(g[k], g64m[k]) / max(rel(g32m[k], g64m[k]), 1e-300) for k in g64m), len(bad), len(g64m)))
    return bad


# ------------------------------------------------------------------------------------- the GPU's own pass and its masks
def gpu_pass(net, batch, loss_fn):
    """One training pass through train.forward_saving / train.backward called directly, so that the gradients and the saved
    activations (the masks) are those of ONE pass.  loss_fn(list of per-pair predictions [N_i,3]) -> scalar.
    Returns (loss, {name: gradient on the CPU}, packed prediction, saved)."""
    from scream_amd import train
    net.train()
    pred, saved = train.forward_saving(net, batch)
    leaf = pred.detach().requires_grad_()
    loss = loss_fn(batch.unpack_src(leaf))
    loss.backward()  # the loss alone: d loss / d prediction, zero on padded rows
    grads = train.backward(net, batch, saved, leaf.grad)
    return loss.item(), {n: g.detach().cpu() for (n, _), g in zip(net.named_parameters(), grads)}, pred.detach(), saved


def gpu_masks(batch, saved, pred, refs):
    """The masks of a GPU pass, one dict per pair: scream_relu_bwd masks with `hid > 0` of the saved FFN hidden layer,
    scream_coor_head_bwd and the relu_bwd of coor_mlp.0 with `h > 0` of the saved relu outputs; the L1 sign is that of
    prediction - refs[p] (refs[p] [N_p,3] on the prediction's device, what the loss compares with)."""
    B, row0, lens = batch.n_pairs, batch.cloud_row0_host, batch.cloud_len_host
    masks = [dict() for _ in range(B)]
    for L in saved["layers"]:
        on = (L.hid > 0).cpu()
        for c in range(L.cb, L.cb + L.n):  # the clouds of this block application: rows of L count from L.r0
            a = int(row0[c]) - L.r0
            key = (L.prefix, "src" if c < B else "tgt")
            assert key not in masks[c % B]
            masks[c % B][key] = on[a:a + int(lens[c])][None]
    for key, h in ((("coor_mlp.0.", "src"), saved["h1"]), (("coor_mlp.2.", "src"), saved["h2"])):
        on = (h > 0).cpu()
        for p in range(B):
            masks[p][key] = on[int(row0[p]):int(row0[p]) + int(lens[p])][None]
    for p, x in enumerate(batch.unpack_src(pred)):
        masks[p]["sign"] = torch.sign(x - refs[p]).cpu()[None]
    return masks


def point_gpu(net, pairs, dev):
    """PointTransformer on the packed batch of `pairs` (make_pair tuples), the loss of the training loop averaged over the
    pairs: (loss, gradients, masks per pair) of one gpu_pass."""
    from scream_amd.packing import PackedBatch
    d = [[t.to(dev) for t in p] for p in pairs]
    batch = PackedBatch.from_pairs([p[0][0] for p in d], [p[1][0] for p in d], [p[3].reshape(3) for p in d])
    loss_fn = lambda preds: torch.stack([net.loss(x[None], p[0], p[2], p[3]) for x, p in zip(preds, d)]).mean()
    loss, g, pred, saved = gpu_pass(net, batch, loss_fn)
    return loss, g, gpu_masks(batch, saved, pred, [O.registered(p[0], p[2], p[3])[0] for p in d])


def dem_gpu(net, samples, dev):
    """point_gpu for DEMTransformer on `samples` (terrain tuples): zero centres, the plain L1 against the sample's dem."""
    from scream_amd.packing import PackedBatch
    d = [[t.to(dev) for t in s] for s in samples]
    batch = PackedBatch.from_pairs([s[0][0] for s in d], [s[1][0] for s in d], [torch.zeros(3, device=dev)] * len(d))
    loss_fn = lambda preds: torch.stack([net.loss(x[None], s[2]) for x, s in zip(preds, d)]).mean()
    loss, g, pred, saved = gpu_pass(net, batch, loss_fn)
    return loss, g, gpu_masks(batch, saved, pred, [s[2][0] for s in d])


def point_module_grads(net, src, tgt, rot, trans, dev):
    """The training loop's way: net(...); net.loss(...); loss.backward().  (loss, {name: param.grad on the CPU})."""
    net.train()
    net.zero_grad(set_to_none=True)
    src_, _, _ = net(src.to(dev), tgt.to(dev), trans.permute(0, 2, 1).to(dev), 1.0)
    assert src_.grad_fn is not None
    loss = net.loss(src_, src.to(dev), rot.to(dev), trans.to(dev))
    loss.backward()
    return loss.item(), {n: p.grad.detach().cpu() for n, p in net.named_parameters()}


def dem_module_grads(net, dsm, coarse, dem, dev):
    net.train()
    net.zero_grad(set_to_none=True)
    dem_, imgs = net(dsm.to(dev), coarse.to(dev), False)
    assert dem_.grad_fn is not None and imgs is None
    loss = net.loss(dem_, dem.to(dev))
    loss.backward()
    return loss.item(), {n: p.grad.detach().cpu() for n, p in net.named_parameters()}


def assert_bitwise(what, a, b):
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), "%s: gradient of %s differs" % (what, k)
