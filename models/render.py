"""Drop-in for the reference's ``models/render.py``: same import path, class name and constructor
(reference models/render.py:8-73), backed by the MI355X kernels in ``scream_amd`` (csrc/render.hip).

    from models.render import RegistrationRender
    gen = RegistrationRender(rho=24, w=64)     # view="single": one view
    imgs = gen(src_pred, tgt)                   # [V, 2, w, w], differentiable in src_pred
"""
from scream_amd.render import RegistrationRender  # noqa: F401

__all__ = ["RegistrationRender"]
