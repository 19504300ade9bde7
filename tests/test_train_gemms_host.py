"""scream_amd.train's arithmetic classes where no GPU is needed: the table against the models' backend names, gemms()'s
refusals, the split GEMM's K rule against its hand-derived values, and the library's own refusal of the K the rule excludes."""
import pytest

from scream_amd import _lib, train
from scream_amd.model import DEMTransformer, PointTransformer

EUNSUPPORTED = -2


def test_one_arithmetic_per_backend_name():
    assert tuple(train.ARITHMETICS) == PointTransformer.TRAIN_BACKENDS == DEMTransformer.TRAIN_BACKENDS
    for name, cls in train.ARITHMETICS.items():
        mm = train.gemms(name)
        assert type(mm) is cls and mm.name == name
        assert all(callable(getattr(mm, m)) for m in ("fwd", "dgrad", "wgrad"))
    assert train.wgrad_split is not train.wgrad and train.wgrad_bf16 is not train.wgrad


@pytest.mark.parametrize("bad", ["h2", None])
def test_gemms_refuses_an_unknown_name_with_the_models_message(bad):
    with pytest.raises(ValueError) as model_says:
        PointTransformer(256, 1, 1).train_backend = bad
    with pytest.raises(ValueError) as gemms_says:
        train.gemms(bad)
    assert str(gemms_says.value) == str(model_says.value) and "'f32', 'split', 'bf16'" in str(gemms_says.value)


def test_the_split_gemm_k_rule():
    """K = 64 + 192 j, i.e. K % 64 == 0 and (K / 32 - 2) % 3 == 0, by hand: 64 -> 0, 256 -> 6, 448 -> 12, 1024 -> 30 are multiples
    of three; 128 -> 2, 512 -> 14, 768 -> 22 are not; 32 is no multiple of 64; 0 is no contraction."""
    for K in (64, 256, 448, 1024):
        assert train.split_gemm_takes_k(K) is True, K
    for K in (0, 32, 128, 512, 768):
        assert train.split_gemm_takes_k(K) is False, K
    assert train.SPLIT_K == 256  # the depth the refused data gradients are cut into is one the rule takes


@pytest.mark.parametrize("K", [512, 768])
def test_the_library_refuses_the_k_the_rule_excludes(K):
    """Only refused shapes: an accepted one would launch.  The pointers are never dereferenced."""
    p = 1 << 20
    rc = _lib.load().scream_gemm_split_f32(p, K, p, p, 256, 128, 256, K, 0, 0, None, None, 0, None, None, 0, _lib.SPLIT_BF3, 0, 0, None)
    assert rc == EUNSUPPORTED
