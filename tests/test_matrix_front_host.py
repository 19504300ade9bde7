"""The refusal contract of the matrix entry points, on the CPU: which argument tuples come back SCREAM_EINVAL (-1), which
SCREAM_EUNSUPPORTED (-2), which one wins when a tuple breaks two rules, and which calls have no work and return 0 before any
launch.

Every expected value below was recorded from a build of the commit BEFORE the host front end of these entry points was shared
(scream_amd/csrc/matrix_front.h, split.h); none was taken from the tree under test.  A row is the entry point's `base` call --
a complete valid call, which is itself never made -- with a few arguments changed so that the call is refused or has nothing to
do.  Pointers are made-up addresses that nothing dereferences; scream_tail_exps_t is a real struct, read on the host.

The module skips itself where a GPU is visible: a row that a broken check let through would launch a kernel on made-up
addresses, and that must not be possible on a machine that others share."""
import ctypes as C

import pytest
import torch

from scream_amd import _lib

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="made-up addresses: never where a kernel could be launched on them")

P, P2 = 0x10000, 0x20000  # aligned made-up addresses
ODD = P + 4               # one that is not 16-byte aligned
EINVAL, EUNSUPPORTED = -1, -2


def exps(**kw):
    e = _lib.TailExpsT()
    for k, v in kw.items():
        assert hasattr(e, k)
        setattr(e, k, v)
    return e


# entry point -> (base call: argument name -> value, in the order of include/scream_hip.h;  rows: (changed arguments, return))
TABLE = {
    "scream_gemm_f32": (
        dict(A=P, lda=256, W=P, C=P, ldc=256, M=128, N=256, K=256, epilogue=0, n_act=0, bias=0, residual=0, ldr=0, gamma=0, beta=0,
             stream=0),
        [(dict(A=0), EINVAL), (dict(W=0), EINVAL), (dict(C=0), EINVAL),
         (dict(M=-128), EUNSUPPORTED), (dict(M=64), EUNSUPPORTED), (dict(N=0), EUNSUPPORTED), (dict(N=128), EUNSUPPORTED),
         (dict(K=0), EUNSUPPORTED), (dict(K=32), EUNSUPPORTED),
         (dict(lda=192), EINVAL), (dict(ldc=128), EINVAL), (dict(lda=258), EINVAL), (dict(ldc=258), EINVAL),
         (dict(A=ODD), EINVAL), (dict(W=ODD), EINVAL), (dict(C=ODD), EINVAL),
         (dict(epilogue=1, n_act=-256), EUNSUPPORTED), (dict(epilogue=1, n_act=128), EUNSUPPORTED),
         (dict(epilogue=3), EINVAL),
         (dict(epilogue=4, N=512, ldc=512, residual=P, gamma=P, beta=P, ldr=512), EUNSUPPORTED),
         (dict(epilogue=4), EINVAL), (dict(epilogue=4, residual=P, beta=P, ldr=256), EINVAL),
         (dict(epilogue=4, residual=P, gamma=P, ldr=256), EINVAL), (dict(epilogue=4, residual=P, gamma=P, beta=P, ldr=128), EINVAL),
         (dict(epilogue=4, residual=P, gamma=P, beta=P, ldr=258), EINVAL),
         (dict(epilogue=4, residual=ODD, gamma=P, beta=P, ldr=256), EINVAL),
         (dict(epilogue=5), EINVAL), (dict(epilogue=6), EINVAL), (dict(epilogue=-1), EINVAL),
         # two rules, two codes
         (dict(A=0, M=64), EINVAL), (dict(M=64, lda=192), EUNSUPPORTED), (dict(K=32, A=ODD), EUNSUPPORTED),
         (dict(epilogue=7, N=128), EUNSUPPORTED), (dict(epilogue=4, N=512, ldc=512), EUNSUPPORTED),
         (dict(epilogue=1, n_act=128, C=ODD), EINVAL),
         # 2^31 output tiles
         (dict(M=1 << 38), EUNSUPPORTED),
         # no work: 0 behind every check
         (dict(M=0), 0), (dict(M=0, epilogue=2), 0), (dict(M=0, epilogue=3), EINVAL), (dict(M=0, epilogue=9), EINVAL)]),
    "scream_gemm_qkv_f32": (
        dict(A=P, lda=256, W=P, Q=P, ldq=256, M=128, N=768, K=256, n_q=256, tile_cloud=P, cloud_row0=P, cloud_len=P, row_base=0,
             kv_partial=P, stream=0),
        [(dict(A=0), EINVAL), (dict(W=0), EINVAL), (dict(kv_partial=0), EINVAL), (dict(tile_cloud=0), EINVAL),
         (dict(cloud_row0=0), EINVAL), (dict(cloud_len=0), EINVAL),
         (dict(M=64), EUNSUPPORTED), (dict(M=-128), EUNSUPPORTED), (dict(N=0), EUNSUPPORTED), (dict(K=32), EUNSUPPORTED),
         (dict(K=0), EUNSUPPORTED),
         (dict(n_q=128), EUNSUPPORTED), (dict(N=1280), EUNSUPPORTED), (dict(N=256), EUNSUPPORTED),
         (dict(n_q=0, N=1024), EUNSUPPORTED),  # several key/value tile pairs: not on the fp32 kernel
         (dict(row_base=-128), EUNSUPPORTED), (dict(row_base=64), EUNSUPPORTED),
         (dict(Q=0), EINVAL), (dict(ldq=128), EINVAL), (dict(ldq=258), EINVAL), (dict(Q=ODD), EINVAL),
         (dict(lda=128), EINVAL), (dict(lda=258), EINVAL), (dict(A=ODD), EINVAL), (dict(W=ODD), EINVAL),
         (dict(Q=0, n_q=128), EUNSUPPORTED), (dict(tile_cloud=0, M=64), EINVAL), (dict(row_base=64, A=ODD), EUNSUPPORTED),
         (dict(M=1 << 38), EUNSUPPORTED),
         (dict(M=0), 0), (dict(M=0, n_q=0, N=512, Q=0, ldq=0), 0), (dict(M=0, lda=128), EINVAL)]),
    "scream_pack_w_split": (
        dict(W=P, N=256, K=64, split=2, w_exp=0, packed=P, stream=0),
        [(dict(W=0), EINVAL), (dict(packed=0), EINVAL), (dict(split=0), EINVAL), (dict(split=4), EINVAL),
         (dict(w_exp=61), EINVAL), (dict(w_exp=-61), EINVAL), (dict(split=1, w_exp=61), EINVAL),
         (dict(N=0), EUNSUPPORTED), (dict(N=6), EUNSUPPORTED), (dict(K=0), EUNSUPPORTED), (dict(K=48), EUNSUPPORTED),
         (dict(W=ODD), EINVAL), (dict(packed=ODD), EINVAL),
         (dict(split=0, N=6), EINVAL), (dict(N=6, W=ODD), EUNSUPPORTED),
         (dict(split=3, w_exp=100, N=6), EUNSUPPORTED)]),  # bf16 x 3 reads no exponent: the shape is what refuses this one
    "scream_gemm_split_f32": (
        dict(A=P, lda=256, W_packed=P, C=P, ldc=256, M=128, N=256, K=256, epilogue=0, n_act=0, bias=0, residual=0, ldr=0, gamma=0,
             beta=0, layout=0, split=2, a_exp=0, w_exp=0, stream=0),
        [(dict(A=0), EINVAL), (dict(W_packed=0), EINVAL), (dict(C=0), EINVAL),
         (dict(split=0), EINVAL), (dict(split=4), EINVAL), (dict(a_exp=61), EINVAL), (dict(a_exp=-61), EINVAL), (dict(w_exp=61), EINVAL),
         (dict(split=1, w_exp=-61), EINVAL),
         (dict(M=-128), EUNSUPPORTED), (dict(M=64), EUNSUPPORTED), (dict(N=0), EUNSUPPORTED), (dict(N=128), EUNSUPPORTED),
         (dict(K=0), EUNSUPPORTED), (dict(K=32), EUNSUPPORTED), (dict(K=128), EUNSUPPORTED), (dict(K=320, lda=320), EUNSUPPORTED),
         (dict(lda=192), EINVAL), (dict(ldc=128), EINVAL), (dict(lda=258), EINVAL), (dict(ldc=258), EINVAL),
         (dict(A=ODD), EINVAL), (dict(W_packed=ODD), EINVAL), (dict(C=ODD), EINVAL),
         (dict(layout=4), EINVAL), (dict(layout=1, lda=512), EUNSUPPORTED), (dict(layout=1, K=64), EUNSUPPORTED),
         (dict(layout=2), EUNSUPPORTED), (dict(layout=2, epilogue=1, n_act=0), EUNSUPPORTED),
         (dict(layout=2, epilogue=1, n_act=256, N=512, ldc=512), EUNSUPPORTED), (dict(layout=2, epilogue=2, n_act=256), EUNSUPPORTED),
         (dict(epilogue=1, n_act=-256), EUNSUPPORTED), (dict(epilogue=1, n_act=128), EUNSUPPORTED),
         (dict(epilogue=3), EINVAL),
         (dict(epilogue=4, N=512, ldc=512, residual=P, gamma=P, beta=P, ldr=512), EUNSUPPORTED),
         (dict(epilogue=4), EINVAL), (dict(epilogue=4, residual=P, beta=P, ldr=256), EINVAL),
         (dict(epilogue=4, residual=P, gamma=P, ldr=256), EINVAL), (dict(epilogue=4, residual=P, gamma=P, beta=P, ldr=128), EINVAL),
         (dict(epilogue=4, residual=P, gamma=P, beta=P, ldr=258), EINVAL),
         (dict(epilogue=4, residual=ODD, gamma=P, beta=P, ldr=256), EINVAL),
         (dict(epilogue=5), EINVAL), (dict(epilogue=6), EINVAL), (dict(epilogue=-1), EINVAL),
         (dict(split=0, M=64), EINVAL), (dict(A=0, K=128), EINVAL), (dict(K=128, lda=64), EUNSUPPORTED),
         (dict(layout=4, epilogue=9), EINVAL), (dict(layout=2, epilogue=9), EUNSUPPORTED), (dict(layout=2, C=ODD), EINVAL),
         (dict(epilogue=4, N=512, ldc=512), EUNSUPPORTED), (dict(split=3, a_exp=99, w_exp=99, M=64), EUNSUPPORTED),
         (dict(M=1 << 39), EUNSUPPORTED),
         (dict(M=0), 0), (dict(M=0, split=3, a_exp=99), 0), (dict(M=0, split=1, epilogue=2), 0), (dict(M=0, epilogue=3), EINVAL)]),
    "scream_gemm_qkv_split_f32": (
        dict(A=P, lda=256, W_packed=P, Q=P, ldq=256, M=128, N=768, K=256, n_q=256, tile_cloud=P, cloud_row0=P, cloud_len=P, row_base=0,
             kv_partial=P, layout=0, split=2, a_exp=0, w_exp=0, k_exp=0, v_exp=0, stream=0),
        [(dict(A=0), EINVAL), (dict(W_packed=0), EINVAL), (dict(kv_partial=0), EINVAL), (dict(tile_cloud=0), EINVAL),
         (dict(cloud_row0=0), EINVAL), (dict(cloud_len=0), EINVAL),
         (dict(split=0), EINVAL), (dict(split=4), EINVAL), (dict(a_exp=61), EINVAL), (dict(w_exp=-61), EINVAL),
         (dict(k_exp=41), EINVAL), (dict(k_exp=-41), EINVAL), (dict(v_exp=41), EINVAL), (dict(v_exp=-41), EINVAL),
         (dict(split=1, v_exp=41), EINVAL),
         (dict(M=64), EUNSUPPORTED), (dict(M=-128), EUNSUPPORTED), (dict(N=0), EUNSUPPORTED), (dict(K=32), EUNSUPPORTED),
         (dict(K=128), EUNSUPPORTED),
         (dict(n_q=128), EUNSUPPORTED), (dict(N=1280), EUNSUPPORTED), (dict(N=256), EUNSUPPORTED), (dict(n_q=0, N=768), EUNSUPPORTED),
         (dict(row_base=-128), EUNSUPPORTED), (dict(row_base=64), EUNSUPPORTED),
         (dict(Q=0), EINVAL), (dict(ldq=128), EINVAL), (dict(ldq=258), EINVAL), (dict(Q=ODD), EINVAL),
         (dict(lda=128), EINVAL), (dict(lda=258), EINVAL), (dict(A=ODD), EINVAL), (dict(W_packed=ODD), EINVAL),
         (dict(layout=2, n_q=0, N=512), EUNSUPPORTED), (dict(layout=4), EINVAL), (dict(layout=1, K=64), EUNSUPPORTED),
         (dict(layout=1, lda=512), EUNSUPPORTED), (dict(layout=2, ldq=512), EUNSUPPORTED),
         (dict(k_exp=41, M=64), EINVAL), (dict(M=64, Q=0), EUNSUPPORTED), (dict(split=3, k_exp=41, v_exp=-99, M=64), EUNSUPPORTED),
         (dict(layout=6, n_q=0, N=512), EUNSUPPORTED), (dict(layout=2, ldq=512, A=ODD), EINVAL),
         (dict(M=1 << 39), EUNSUPPORTED),
         (dict(M=0), 0), (dict(M=0, n_q=0, N=1024, Q=0, ldq=0), 0), (dict(M=0, split=3, k_exp=77), 0), (dict(M=0, layout=4), EINVAL)]),
    "scream_proj_image_bytes": (
        dict(N=768, split=2),
        [(dict(split=3), EINVAL), (dict(split=0), EINVAL), (dict(N=0), EINVAL), (dict(N=96), EINVAL), (dict(N=-64, split=1), EINVAL)]),
    "scream_pack_proj": (
        dict(W=P, N=768, n_q=256, split=2, w_exp=0, image=P, stream=0),
        [(dict(W=0), EINVAL), (dict(image=0), EINVAL), (dict(split=3), EINVAL), (dict(split=0), EINVAL),
         (dict(n_q=128), EUNSUPPORTED), (dict(N=256), EUNSUPPORTED), (dict(N=1000), EUNSUPPORTED), (dict(n_q=0), EUNSUPPORTED),
         (dict(w_exp=61), EINVAL), (dict(w_exp=-61), EINVAL), (dict(image=ODD), EINVAL),
         (dict(split=3, n_q=128), EINVAL), (dict(n_q=128, w_exp=61), EUNSUPPORTED), (dict(N=1000, image=ODD), EUNSUPPORTED)]),
    "scream_proj_qkv_f32": (
        dict(x=P, proj_image=P, Q=P, M=128, N=768, n_q=256, tile_cloud=P, cloud_row0=P, cloud_len=P, row_base=0, kv_partial=P, split=2,
             a_exp=0, w_exp=0, k_exp=0, v_exp=0, stream=0),
        [(dict(x=0), EINVAL), (dict(proj_image=0), EINVAL), (dict(kv_partial=0), EINVAL), (dict(tile_cloud=0), EINVAL),
         (dict(cloud_row0=0), EINVAL), (dict(cloud_len=0), EINVAL), (dict(split=3), EINVAL), (dict(split=0), EINVAL),
         (dict(n_q=128), EUNSUPPORTED), (dict(N=1280), EUNSUPPORTED), (dict(N=256), EUNSUPPORTED), (dict(n_q=0), EUNSUPPORTED),
         (dict(M=64), EUNSUPPORTED), (dict(M=-128), EUNSUPPORTED), (dict(row_base=64), EUNSUPPORTED), (dict(row_base=-128), EUNSUPPORTED),
         (dict(Q=0), EINVAL),
         (dict(a_exp=61), EINVAL), (dict(a_exp=-61), EINVAL), (dict(w_exp=61), EINVAL), (dict(w_exp=-61), EINVAL),
         (dict(k_exp=41), EINVAL), (dict(k_exp=-41), EINVAL), (dict(v_exp=41), EINVAL), (dict(v_exp=-41), EINVAL),
         (dict(a_exp=60, w_exp=60, v_exp=-40), EINVAL), (dict(a_exp=-60, w_exp=-60, v_exp=40), EINVAL),  # v_exp - a_exp - w_exp = -+160
         (dict(x=ODD), EINVAL), (dict(proj_image=ODD), EINVAL), (dict(Q=ODD), EINVAL), (dict(kv_partial=ODD), EINVAL),
         (dict(n_q=0, N=512, Q=ODD), EINVAL),  # Q is asked to be aligned even where there are no queries
         (dict(split=3, M=64), EINVAL), (dict(M=64, a_exp=61), EUNSUPPORTED), (dict(n_q=128, Q=0), EUNSUPPORTED),
         (dict(x=0, row_base=64), EINVAL),
         (dict(M=0), 0), (dict(M=0, n_q=0, N=1024, Q=0), 0), (dict(M=0, split=1), 0), (dict(M=0, a_exp=61), EINVAL)]),
    "scream_tail_image_bytes": (
        dict(split=2, with_next_q=0),
        [(dict(split=0), EINVAL), (dict(split=4), EINVAL), (dict(split=3, with_next_q=1), EINVAL), (dict(split=-1, with_next_q=1), EINVAL)]),
    "scream_pack_tail": (
        dict(Wm=P, W1=P, W2=P, Wq_next=0, split=2, exps=exps(), image=P, stream=0),
        [(dict(Wm=0), EINVAL), (dict(W1=0), EINVAL), (dict(W2=0), EINVAL), (dict(image=0), EINVAL), (dict(split=0), EINVAL),
         (dict(split=4), EINVAL), (dict(Wq_next=P, split=3), EUNSUPPORTED), (dict(image=ODD), EINVAL),
         (dict(exps=None), EINVAL), (dict(split=1, exps=None), EINVAL),
         (dict(exps=exps(e_att=41)), EINVAL), (dict(exps=exps(e_wm=-41)), EINVAL), (dict(exps=exps(e_m1=41)), EINVAL),
         (dict(exps=exps(e_w1=-41)), EINVAL), (dict(exps=exps(e_h=41)), EINVAL), (dict(exps=exps(e_w2=-41)), EINVAL),
         (dict(exps=exps(e_q=-41)), EINVAL), (dict(exps=exps(e_q=41)), EINVAL), (dict(exps=exps(e_y=41)), EINVAL),
         (dict(exps=exps(e_wq=-41)), EINVAL),
         (dict(exps=exps(e_wm=30, e_att=30)), EINVAL), (dict(exps=exps(e_w2=-30, e_h=-30)), EINVAL),  # e_wm + e_att, e_w2 + e_h: +-44
         (dict(exps=exps(e_h=40, e_w1=-40, e_m1=-40)), EINVAL), (dict(exps=exps(e_h=-40, e_w1=40, e_m1=40)), EINVAL),  # +-100
         (dict(Wq_next=P, split=3, image=ODD), EUNSUPPORTED), (dict(Wq_next=P, split=0), EINVAL),
         (dict(Wq_next=P, split=3, exps=None, Wm=0), EINVAL)]),
    "scream_kv_finalize_image": (
        dict(kv_partial=P, cloud_row0=P, cloud_len=P, row_base=0, cloud_begin=0, n_kv=1, kv_image=P, n_layers=1, partial_layer_stride=0,
             image_layer_stride=0, split=2, stream=0),
        [(dict(kv_partial=0), EINVAL), (dict(cloud_row0=0), EINVAL), (dict(cloud_len=0), EINVAL), (dict(kv_image=0), EINVAL),
         (dict(split=0), EINVAL), (dict(split=4), EINVAL),
         (dict(n_kv=-1), EINVAL), (dict(cloud_begin=-1), EINVAL), (dict(row_base=-1), EINVAL), (dict(n_layers=0), EINVAL),
         (dict(n_layers=65536, partial_layer_stride=1024, image_layer_stride=1024), EINVAL),
         (dict(n_layers=2), EINVAL), (dict(n_layers=2, partial_layer_stride=1024), EINVAL),
         (dict(n_layers=2, partial_layer_stride=1024, image_layer_stride=24), EINVAL),
         (dict(kv_image=ODD), EINVAL), (dict(kv_partial=ODD), EINVAL), (dict(partial_layer_stride=6), EINVAL),
         (dict(n_kv=0), 0), (dict(n_kv=0, split=3, n_layers=2, partial_layer_stride=1024, image_layer_stride=1024), 0),
         (dict(n_kv=0, split=0), EINVAL)]),
    "scream_layer_tail_f32": (
        dict(Q=P, kv_image=P, tile_cloud=P, kv_cloud_offset=0, cloud_len=P, x=P, tail_image=P, g1=P, b1=P, g2=P, b2=P, y=P2, q_next=0,
             M=128, split=2, exps=exps(), stream=0),
        [(dict(Q=0), EINVAL), (dict(kv_image=0), EINVAL), (dict(tile_cloud=0), EINVAL), (dict(cloud_len=0), EINVAL), (dict(x=0), EINVAL),
         (dict(tail_image=0), EINVAL), (dict(g1=0), EINVAL), (dict(b1=0), EINVAL), (dict(g2=0), EINVAL), (dict(b2=0), EINVAL),
         (dict(y=0), EINVAL), (dict(split=0), EINVAL), (dict(split=4), EINVAL),
         (dict(M=64), EUNSUPPORTED), (dict(M=-128), EUNSUPPORTED),
         (dict(Q=ODD), EINVAL), (dict(kv_image=ODD), EINVAL), (dict(x=ODD), EINVAL), (dict(tail_image=ODD), EINVAL), (dict(g1=ODD), EINVAL),
         (dict(b1=ODD), EINVAL), (dict(g2=ODD), EINVAL), (dict(b2=ODD), EINVAL), (dict(y=ODD), EINVAL), (dict(q_next=ODD), EINVAL),
         (dict(y=P), EINVAL),  # x == y
         (dict(q_next=0x30000, split=3), EINVAL), (dict(q_next=P), EINVAL), (dict(q_next=P2), EINVAL),  # bf16 x 3 / == x / == y
         (dict(exps=None), EINVAL), (dict(split=1, exps=None), EINVAL), (dict(exps=exps(e_att=41)), EINVAL),
         (dict(exps=exps(e_y=-41)), EINVAL), (dict(exps=exps(e_wm=30, e_att=30)), EINVAL),
         (dict(split=0, M=64), EINVAL), (dict(M=64, y=P), EUNSUPPORTED), (dict(M=64, exps=None), EUNSUPPORTED),
         (dict(Q=0, M=-128), EINVAL),
         (dict(M=1 << 38), EUNSUPPORTED),
         (dict(M=0), 0), (dict(M=0, split=3, exps=None), 0), (dict(M=0, q_next=0x30000), 0), (dict(M=0, exps=None), EINVAL)]),
    "scream_act_layout": (
        dict(src=P, dst=P2, M=32, to_fragment=1, stream=0),
        [(dict(src=0), EINVAL), (dict(dst=0), EINVAL), (dict(dst=P), EINVAL), (dict(M=-32), EUNSUPPORTED), (dict(M=16), EUNSUPPORTED),
         (dict(M=32 << 31), EUNSUPPORTED), (dict(src=ODD), EINVAL), (dict(dst=ODD), EINVAL),
         (dict(src=0, M=16), EINVAL), (dict(M=16, src=ODD), EUNSUPPORTED),
         (dict(M=0), 0), (dict(M=0, to_fragment=0), 0), (dict(M=0, dst=ODD), EINVAL)]),
    # (wgrad_run's last clause, more than 65535 row slices, cannot be reached: the carve hands out at most 1024)
    "scream_gemm_wgrad_split_f32": (
        dict(dY=P, ldy=128, X=P, ldx=128, rows=128, N=128, K=128, dW=P, accumulate=1, colsum=0, split=3, workspace=P,
             workspace_bytes=1 << 40, stream=0),
        [(dict(split=2), EINVAL), (dict(split=1), EINVAL), (dict(split=0), EINVAL), (dict(split=4), EINVAL),
         (dict(dY=0), EINVAL), (dict(X=0), EINVAL), (dict(dW=0), EINVAL),
         (dict(rows=-1), EUNSUPPORTED), (dict(N=0), EUNSUPPORTED), (dict(K=0), EUNSUPPORTED), (dict(N=64), EUNSUPPORTED),
         (dict(K=200), EUNSUPPORTED),
         (dict(ldy=64), EINVAL), (dict(ldx=64), EINVAL), (dict(ldy=130), EINVAL), (dict(ldx=130), EINVAL), (dict(dY=ODD), EINVAL),
         (dict(X=ODD), EINVAL),
         (dict(workspace=0), EINVAL), (dict(workspace_bytes=0), EINVAL), (dict(workspace=ODD), EINVAL),
         (dict(split=2, N=64), EINVAL), (dict(N=64, ldy=2), EUNSUPPORTED), (dict(dY=0, K=200), EINVAL),
         (dict(rows=0), 0), (dict(rows=0, colsum=P, workspace=0, workspace_bytes=0), 0), (dict(rows=0, split=2), EINVAL)]),
}


def _call(lib, name, args):
    vals = [C.byref(v) if isinstance(v, _lib.TailExpsT) else v for v in args.values()]
    return getattr(lib, name)(*vals)


def test_the_table_covers_the_matrix_entry_points_and_makes_no_complete_call():
    assert len(TABLE) == 14
    for name, (base, rows) in TABLE.items():
        assert len(base) == len(_lib.SIGNATURES[name][1]), name
        assert len(rows) >= 4, name
        for changed, rc in rows:
            assert changed and set(changed) <= set(base), (name, changed)
            assert rc in (0, EINVAL, EUNSUPPORTED), (name, changed)
            assert any(base[k] is not v and base[k] != v for k, v in changed.items()), (name, changed)
        if name.endswith("_image_bytes"):
            continue
        # both codes, and (where the entry point has one) a call with no work
        assert {EINVAL, EUNSUPPORTED} <= {rc for _, rc in rows} or name == "scream_kv_finalize_image", name
    no_work = [n for n, (_, rows) in TABLE.items() if any(rc == 0 for _, rc in rows)]
    assert sorted(no_work) == ["scream_act_layout", "scream_gemm_f32", "scream_gemm_qkv_f32", "scream_gemm_qkv_split_f32",
                               "scream_gemm_split_f32", "scream_gemm_wgrad_split_f32", "scream_kv_finalize_image",
                               "scream_layer_tail_f32", "scream_proj_qkv_f32"]


@pytest.mark.parametrize("name", sorted(TABLE))
def test_refusals_are_what_they_were(name):
    lib = _lib.load()
    base, rows = TABLE[name]
    got = [(changed, _call(lib, name, {**base, **changed})) for changed, _ in rows]
    wrong = [(changed, rc, want) for (changed, rc), (_, want) in zip(got, rows) if rc != want]
    assert not wrong, "%s: (changed arguments, returned, recorded) %r" % (name, wrong)
