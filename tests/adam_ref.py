"""The Adam contract of include/scream_hip.h ("The optimiser step") restated in numpy: fp32 state, every step one IEEE float64
operation in the header's order, one rounding per stored value, the running powers of the betas, the skipped step.  numpy's
float64 +, -, *, / and sqrt are correctly rounded, so a device that rounds its float64 square root and divisions correctly
gives these bits.

    ref = AdamRef([p0, p1, ...], lr=2e-4)                # numpy arrays (any shape); copies are kept as fp32
    ref.step([g0, None, ...])                            # None: that parameter is skipped
    ref.step(grads, grad_scale=65536.0, found_inf=0.0)   # a GradScaler's step; found_inf != 0 changes nothing

``state=np.float64`` keeps p, m and v in float64 instead (no rounding anywhere): the all-float64 trajectory that fp32 paths are
measured against."""
import math

import numpy as np


def running_powers(b1, b2, steps):
    q1 = q2 = 1.0
    for _ in range(int(steps)):
        q1 *= b1
        q2 *= b2
    return q1, q2


class AdamRef:
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, state=np.float32):
        self.dtype = np.dtype(state)
        self.p = [np.array(p, dtype=np.float32).astype(self.dtype) for p in params]
        self.m = [np.zeros_like(p) for p in self.p]
        self.v = [np.zeros_like(p) for p in self.p]
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        self.q1, self.q2, self.steps = 1.0, 1.0, 0

    def load(self, m, v, steps):
        """The state a torch.optim.Adam holds after `steps` steps."""
        self.m = [np.array(a, dtype=np.float32).astype(self.dtype) for a in m]
        self.v = [np.array(a, dtype=np.float32).astype(self.dtype) for a in v]
        self.steps = int(steps)
        self.q1, self.q2 = running_powers(self.betas[0], self.betas[1], steps)

    def step(self, grads, grad_scale=None, found_inf=None, lr=None):
        if found_inf is not None and float(found_inf) != 0.0:
            return
        lr = self.lr if lr is None else float(lr)
        b1, b2 = self.betas
        inv = 1.0 if grad_scale is None else 1.0 / float(np.float64(np.float32(grad_scale)))
        q1, q2 = self.q1 * b1, self.q2 * b2
        step_size = lr / (1.0 - q1)
        sqrt_bc2 = math.sqrt(1.0 - q2)
        one_b1, one_b2 = 1.0 - b1, 1.0 - b2
        with np.errstate(all="ignore"):
            for i, g32 in enumerate(grads):
                if g32 is None:
                    continue
                g = np.asarray(g32, dtype=np.float32).astype(np.float64) * inv
                p, m, v = (a[i].astype(np.float64) for a in (self.p, self.m, self.v))
                m1 = m + (g - m) * one_b1
                v1 = (b2 * v) + (one_b2 * (g * g))
                denom = np.sqrt(v1) / sqrt_bc2 + self.eps
                p1 = p - step_size * (m1 / denom)
                self.p[i], self.m[i], self.v[i] = p1.astype(self.dtype), m1.astype(self.dtype), v1.astype(self.dtype)
        self.q1, self.q2, self.steps = q1, q2, self.steps + 1
