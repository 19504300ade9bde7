"""Training surface that needs no GPU: the train() switch of PointTransformer and the host-side checks of the backward
entry points (include/scream_hip.h, ABI 21)."""
import torch

from scream_amd import _lib
from scream_amd.model import PointTransformer


def test_explicit_train_switches_the_forward_to_the_training_path():
    net = PointTransformer(256, 1, 1)
    assert net.training and not net._trains()  # nn.Module starts in training mode; that alone keeps the inference path
    net.train()
    assert net._trains()
    with torch.no_grad():
        assert not net._trains()
    net.eval()
    assert not net._trains()
    assert net.train(True) is net and net._trains()
    net.train(False)
    assert not net._trains() and not net.training


def test_backward_entry_points_check_their_arguments_on_the_host():
    lib = _lib.load()
    assert _lib.ABI_VERSION == 21 and lib.scream_abi_version() == 21
    # weight gradient: one partial slab of N x K (+ N column sums) per row slice
    ws = lib.scream_wgrad_workspace_bytes(330000, 256, 256)
    assert ws > 0 and ws % ((256 * 256 + 256) * 4) == 0
    assert lib.scream_wgrad_workspace_bytes(128, 256, 256) == (256 * 256 + 256) * 4  # one slice
    assert lib.scream_wgrad_workspace_bytes(128, 200, 256) == -1
    assert lib.scream_gemm_wgrad_f32(None, 256, None, 256, 128, 256, 256, None, 0, None, None, 0, None) == -1
    assert lib.scream_ln_bwd_workspace_bytes(1024) == 2 * 2 * 256 * 4
    assert lib.scream_attn_bwd_workspace_bytes(2, 3) == 2 * 4 * 8 * 1056 * 4
    assert lib.scream_grad3_workspace_bytes(513) == 2 * (4 * 256 + 4) * 4
    assert lib.scream_relu_bwd(None, None, 4, None) == -1
    assert lib.scream_ln_fwd(None, None, None, None, None, None, None, 128, None) == -1
