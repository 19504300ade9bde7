"""Depth renderer (scream_amd/render.py, csrc/render.hip) without a GPU: the restatement in tests/render_ref.py against the
reference's own module, the view matrices against scipy, the models' generator, and the host-side checks of the new entry points."""
import importlib.util
import os
import sys
import types

import numpy as np
import pytest
import torch

import render_ref as RR
from scream_amd import _lib
from scream_amd.render import RegistrationRender, rotation_matrix, view_eulers

REF_RENDER = os.path.join(os.environ.get("SCREAM_REFERENCE", "/root/reference"), "models", "render.py")  # as oracle/make_golden.py


def _reference_renderer(rho, w, view="muti"):
    """The reference's RegistrationRender loaded by file path under a private name (the repository's own `models` package would
    shadow it), built without its __init__ (which hard-codes cuda:0) and set up as render.py:11-25 do, on the CPU."""
    if "cv2" not in sys.modules:
        sys.modules["cv2"] = types.ModuleType("cv2")  # imported by render.py, never used by the renderer
    spec = importlib.util.spec_from_file_location("_scream_reference_render", REF_RENDER)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    obj = mod.RegistrationRender.__new__(mod.RegistrationRender)
    torch.nn.Module.__init__(obj)
    obj.rho, obj.w = rho, w
    i, j = np.arange(w * w) // w, np.arange(w * w) % w
    pix_xy = torch.from_numpy(np.concatenate([j.reshape(-1, 1), i.reshape(-1, 1)], axis=1)).float()
    obj.pix_xy = (pix_xy - w // 2 + 0.5) / (w // 2)
    obj.eulers = view_eulers(view)
    return obj


def _clouds(n, m, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, 3, generator=g) * 1.6 - 0.8, torch.rand(m, 3, generator=g) * 1.6 - 0.8


@pytest.mark.skipif(not os.path.exists(REF_RENDER), reason="the reference is not on this machine")
@pytest.mark.parametrize("w,view", [(64, "muti"), (128, "single")])
def test_restatement_equals_the_reference_renderer(w, view):
    pytest.importorskip("scipy")
    ref = _reference_renderer(24, w, view)
    src, tgt = _clouds(120, 90)
    src.requires_grad_(True)
    want = ref(src, tgt)
    got, amax, _ = RR.render(src.detach(), tgt, 24, w, ref.eulers)
    assert torch.equal(got, want.detach())  # bit for bit in fp32
    # gradient of a random linear loss: torch's autograd through the reference vs the analytic backward under the restatement's
    # argmax, on pixels where the source image has no tie (torch's max routes a tie to one of the points; the rule is documented)
    up = torch.randn(want.shape, generator=torch.Generator().manual_seed(1))
    _, _, _, gap = RR.render(src.detach(), tgt, 24, w, ref.eulers, top2=True)
    up[:, 0][gap[:, 0] == 0] = 0.0
    up[:, 1] = 0.0
    g_ref = torch.autograd.grad((want * up).sum(), src)[0]
    g_ana = RR.backward(src.detach(), tgt, up, amax, 24, w, ref.eulers, dtype=torch.float32)
    assert g_ref.abs().max() > 0
    torch.testing.assert_close(g_ana, g_ref, rtol=2e-5, atol=1e-6 * g_ref.abs().max().item())


@pytest.mark.skipif(not os.path.exists(REF_RENDER), reason="the reference is not on this machine")
def test_restatement_reassigned_eulers_follow_the_reference():
    pytest.importorskip("scipy")
    ref = _reference_renderer(24, 64)
    ref.eulers = [np.array([0.3, -1.1, 2.0]), np.array([0, 0, np.pi / 4])]
    src, tgt = _clouds(50, 70, seed=3)
    assert torch.equal(RR.render(src, tgt, 24, 64, ref.eulers)[0], ref(src, tgt))


def test_split_plan_restates_the_host_rule():
    # the B = 32 training step at w = 64, six views: 4 tiles * 384 images = 1536 blocks -> ceil(2048 / 1536) = 2 splits
    assert RR.split_plan(64, 32, 6, 5100) == (2, 2550)
    # one pair: 48 blocks -> 43 splits wanted, ceil(5000 / 256) = 20 allowed
    assert RR.split_plan(64, 1, 6, 5000) == (20, 250)
    # the other calls of tests/test_gpu_render.py: none reaches 768 staged points before its range ends
    assert RR.split_plan(128, 1, 6, 5000) == (11, 455)  # 192 blocks -> 11 splits
    assert RR.split_plan(64, 5, 6, 5000) == (9, 556)    # 240 blocks -> 9 splits
    assert RR.split_plan(64, 1, 1, 16000) == (63, 254)  # 8 blocks -> 256 wanted, 63 allowed; ceil(16000 / 63) = 254
    # the shapes of tests/test_gpu_render_paths.py
    assert RR.split_plan(64, 16, 6, 7500) == (3, 2500)  # 768 blocks
    assert RR.split_plan(256, 16, 1, 3000) == (1, 3000)  # 2048 blocks: no split at all
    assert RR.split_plan(256, 1, 6, 4000) == (3, 1334)  # 768 blocks; 3 * 1334 = 4002
    assert RR.split_plan(192, 1, 1, 1500) == (6, 250)
    assert RR.split_plan(64, 1, 6, 1) == (1, 1)
    # per_split is rounded up: 576 blocks -> 4 splits of ceil(1025 / 4) = 257 (the last one holds 254 points)
    assert RR.split_plan(64, 12, 6, 1025) == (4, 257)
    assert RR.split_plan(64, 12, 6, 1030) == (4, 258)


def test_restatement_in_point_chunks_changes_nothing(monkeypatch):
    src, tgt = _clouds(120, 90, seed=5)
    src = torch.cat([src, src[:20]])  # ties across chunks: the lower chunk keeps them, as one chunk's torch.max does here
    want = RR.render(src, tgt, 24, 64, view_eulers("muti")[:2], top2=True)
    monkeypatch.setattr(RR, "POINT_CHUNK", 37)
    got = RR.render(src, tgt, 24, 64, view_eulers("muti")[:2], top2=True)
    assert torch.equal(got[0], want[0]) and torch.equal(got[3], want[3]) and got[2] == want[2]
    assert torch.equal(got[1][:, 1], want[1][:, 1])  # the target has no duplicates
    moved = got[1][:, 0] != want[1][:, 0]
    assert torch.equal(src[got[1][:, 0][moved]], src[want[1][:, 0][moved]])  # a tie may name either copy of the point


def test_view_matrices_equal_scipy_bitwise():
    Rotation = pytest.importorskip("scipy.spatial.transform").Rotation
    rng = np.random.default_rng(0)
    eulers = view_eulers("muti") + view_eulers("single") + [rng.uniform(-7, 7, 3) for _ in range(200)]
    for e in eulers:
        assert torch.equal(rotation_matrix(e), torch.Tensor(Rotation.from_euler('zyx', e).as_matrix())), e


def test_renderer_has_no_state_and_consumes_no_rng():
    torch.manual_seed(0)
    before = torch.get_rng_state()
    gen = RegistrationRender(rho=24, w=64)
    assert torch.equal(before, torch.get_rng_state())
    assert list(gen.parameters()) == [] and list(gen.buffers()) == [] and gen.state_dict() == {}
    assert len(gen.eulers) == 6 and len(RegistrationRender(24, 64, view="single").eulers) == 1
    gen.eulers = gen.eulers[:2]  # a public attribute: the matrices follow it
    assert gen.view_matrices().shape == (2, 3, 3)
    with pytest.raises(ValueError):
        RegistrationRender(24, 100)


def test_models_have_a_parameter_free_generator_and_unchanged_state_dict():
    from scream_amd.model import DEMTransformer, PointTransformer
    from scream_amd.synthetic import dem_state_dict_keys, state_dict_keys
    from models.render import RegistrationRender as Shim
    net = PointTransformer(256, 2, 1)
    assert isinstance(net.generator, Shim) and len(net.generator.eulers) == 6
    assert (net.generator.rho, net.generator.w) == (24, 64)
    assert [(k, tuple(v.shape)) for k, v in net.state_dict().items()] == [(k, tuple(s)) for k, s in state_dict_keys(256, 2, 1)]
    dem = DEMTransformer(256, 2, 1)
    assert isinstance(dem.generator, RegistrationRender) and len(dem.generator.eulers) == 1
    assert [(k, tuple(v.shape)) for k, v in dem.state_dict().items()] == [(k, tuple(s)) for k, s in dem_state_dict_keys(256, 2, 1)]


def test_renderer_on_cpu_tensors_raises():
    src, tgt = _clouds(10, 10)
    with pytest.raises(_lib.ScreamHipError):
        RegistrationRender(24, 64)(src, tgt)


def test_render_entry_points_check_their_arguments_on_the_host():
    lib = _lib.load()
    ws = lib.scream_render_workspace_bytes(1, 6, 64, 5000)
    assert ws >= 6 * 2 * 64 * 64 * 8 and ws >= 6 * 5000 * 3 * 4
    assert lib.scream_render_workspace_bytes(1, 6, 96, 10) == -1  # w % 64 != 0
    assert lib.scream_render_workspace_bytes(1, 0, 64, 10) == -1  # no view
    assert lib.scream_render_workspace_bytes(-1, 6, 64, 10) == -1
    buf = torch.zeros(ws // 4 + 16, dtype=torch.float32)  # host memory: every call below must return before touching it
    p = buf.data_ptr()
    ok = dict(src=p, s_row0=p, s_len=p, tgt=p, t_row0=p, t_len=p, n_pairs=1, max_s=8, max_t=8, rows=8, rot=p, V=6, w=64, rho=24.0,
              imgs=p, argmax=p, ws=p, ws_bytes=lib.scream_render_workspace_bytes(1, 6, 64, 8))

    def fwd(**kw):
        a = dict(ok, **kw)
        return lib.scream_render_depth(a["src"], a["s_row0"], a["s_len"], a["tgt"], a["t_row0"], a["t_len"], a["n_pairs"], a["max_s"],
                                       a["max_t"], a["rows"], a["rot"], a["V"], a["w"], a["rho"], a["imgs"], a["argmax"], a["ws"],
                                       a["ws_bytes"], None)

    def bwd(**kw):
        a = dict(ok, **kw)
        return lib.scream_render_depth_bwd(a["src"], a["s_row0"], a["s_len"], a["n_pairs"], a["max_s"], a["rows"], a["rot"], a["V"],
                                           a["w"], a["rho"], a["imgs"], a["argmax"], a["ws"], a["ws_bytes"], a["imgs"], None)

    for f in (fwd, bwd):
        assert f(w=96) == -1
        assert f(w=0) == -1
        assert f(V=0) == -1
        assert f(src=None) == -1
        assert f(argmax=None) == -1
        assert f(ws=None) == -1
        assert f(ws_bytes=ok["ws_bytes"] - 1) == -1
        assert f(rho=float("nan")) == -1
        assert f(n_pairs=-1) == -1
    assert fwd(tgt=None) == -1 and fwd(imgs=None) == -1
    assert fwd(n_pairs=40000) == -1  # the workspace of one pair
    assert fwd(n_pairs=6000, ws_bytes=lib.scream_render_workspace_bytes(6000, 6, 64, 8)) == -2  # n_pairs * V * 2 > 65535
