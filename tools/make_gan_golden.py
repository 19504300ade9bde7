"""Record tests/golden/gan.npz: what the reference's own discriminator (models/gan.py, NLayerDiscriminator) computes in float64 on
the CPU for one small case, so that tests/test_gan_host.py can hold tests/gan_ref.py without the reference.

    python tools/make_gan_golden.py --reference /path/to/SCREAM --out tests/golden/gan.npz

The case: NLayerDiscriminator(input_nc=2, ndf=8, n_layers=3) in train mode on two 24 x 27 images (convolution outputs 12 x 13,
6 x 6, 3 x 3, 2 x 2, 1 x 1), differentiated for the upstream gradient `dlogits`.  Only data is written: the state dict before the
pass (the weights as int8 codes c, value c / 64, so that they are exact in every float format), the input, dlogits, the logits,
the gradient of the input and of every parameter, and the running statistics after the pass; all results in float64.  To keep
the file small the two largest weight gradients are recorded at every ROW_STEP[name]-th output channel only (every output channel
goes through the same arithmetic; with a reference checkout present tests/test_gan_host.py compares all of them live).
"""
import argparse
import importlib.util
import os

import numpy as np
import torch

N, CIN, NDF, H, W = 2, 2, 8, 24, 27
SCALE = 64.0
ROW_STEP = {"main.5.weight": 4, "main.8.weight": 16}  # output channels kept of the large weight gradients


def load_reference(root):
    spec = importlib.util.spec_from_file_location("reference_models_gan", os.path.join(root, "models", "gan.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="a checkout of the reference (xujiabo/SCREAM)")
    ap.add_argument("--out", default=os.path.join("tests", "golden", "gan.npz"))
    a = ap.parse_args(argv)
    ref = load_reference(a.reference)
    net = ref.NLayerDiscriminator(input_nc=CIN, ndf=NDF, n_layers=3, use_actnorm=False).double().train()
    rng = np.random.default_rng(20)
    out = {}
    sd = net.state_dict()
    for name, t in sd.items():
        if name.endswith("num_batches_tracked"):
            continue
        code = rng.integers(-16, 17, size=tuple(t.shape)).astype(np.int8)
        offset = 1.0 if name.endswith("running_var") or (t.dim() == 1 and name.endswith("weight")) else 0.0  # BatchNorm scale, variance
        if name.endswith("running_var"):
            code = np.abs(code)
        out["code." + name] = code
        out["offset." + name] = np.float64(offset)
        sd[name] = torch.from_numpy(offset + code.astype(np.float64) / SCALE)
    net.load_state_dict(sd)
    x = rng.standard_normal((N, CIN, H, W)).astype(np.float32)
    xt = torch.from_numpy(x).double().requires_grad_(True)
    logits = net(xt)
    dlogits = rng.standard_normal(tuple(logits.shape)).astype(np.float32)
    (logits * torch.from_numpy(dlogits).double()).sum().backward()
    out.update(x=x, dlogits=dlogits, logits=logits.detach().numpy(), dx=xt.grad.numpy())
    for name, p in net.named_parameters():
        out["grad." + name] = p.grad.numpy()[::ROW_STEP.get(name, 1)]
    for name, t in net.state_dict().items():
        if "running_" in name or name.endswith("num_batches_tracked"):
            out["after." + name] = t.numpy()
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    np.savez_compressed(a.out, **out)
    print("wrote %s: %d arrays, %d bytes" % (a.out, len(out), os.path.getsize(a.out)))


if __name__ == "__main__":
    main()
