"""DEMTransformer's training surface that needs no GPU: the train() / eval() / no_grad switch and the layer prefixes the
training forward and backward are built from (scream_amd/train.py)."""
import pytest
import torch

from scream_amd import _lib, train
from scream_amd.model import DEMTransformer, PointTransformer
from scream_amd.packing import PackedBatch


def test_explicit_train_switches_the_dem_forward_to_the_training_path():
    net = DEMTransformer(256, 1, 1)
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


def _owners(net):
    stem, stem_tgt, cross = train._layer_prefixes(net)
    return stem, stem_tgt, cross, stem + (stem_tgt or []) + cross + ["embedding.", "pre_norm.", "coor_mlp."]


def test_dem_layer_prefixes_cover_every_parameter_once():
    for ns, nc in ((1, 1), (2, 3), (6, 6)):
        net = DEMTransformer(256, ns, nc)
        stem, stem_tgt, cross, owners = _owners(net)
        assert stem == ["stem_dsm.%d." % i for i in range(ns)]
        assert stem_tgt == ["stem_dem.%d." % i for i in range(ns)]
        assert cross == [("cross.%d." % j) if j % 2 == 0 else ("cross.%d.layer." % j) for j in range(2 * nc)]
        names = [n for n, _ in net.named_parameters()]
        for n in names:
            assert sum(n.startswith(o) for o in owners) == 1, n
        if (ns, nc) == (6, 6):
            assert len(names) == 250


def test_point_transformer_prefixes_are_unchanged():
    net = PointTransformer(256, 2, 2)
    stem, stem_tgt, cross, owners = _owners(net)
    assert stem == ["stem.0.", "stem.1."] and stem_tgt is None
    assert cross == ["cross.0.", "cross.1.layer.", "cross.2.", "cross.3.layer."]
    for n, _ in net.named_parameters():
        assert sum(n.startswith(o) for o in owners) == 1, n


def _cpu_batch(src_len, tgt_len):
    B = len(src_len)
    lens, row0, rs, rt, tile_cloud, max_chunks = PackedBatch.layout(src_len, tgt_len)
    z = torch.zeros(1)
    return PackedBatch(B, src_len, tgt_len, row0, lens, rs, rt, max_chunks, z, z, z, z, z)


def test_stem_passes_split_the_rows_and_clouds_per_side():
    batch = _cpu_batch([129, 5, 300], [40, 700, 1])
    rs, rt = batch.rows_src, batch.rows_total
    assert train._stem_passes(PointTransformer(256, 2, 1), batch) == [[("stem.0.", 0, rt, 0, 6)], [("stem.1.", 0, rt, 0, 6)]]
    passes = train._stem_passes(DEMTransformer(256, 2, 1), batch)
    assert passes == [[("stem_dsm.%d." % i, 0, rs, 0, 3), ("stem_dem.%d." % i, rs, rt - rs, 3, 3)] for i in range(2)]
    assert rs % 128 == 0 and (rt - rs) % 128 == 0


def test_dem_training_refuses_cpu_parameters():
    net = DEMTransformer(256, 1, 1).train()
    with pytest.raises(_lib.ScreamHipError):
        train.apply(net, None)
