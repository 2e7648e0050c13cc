"""Host-side logic of the unsupervised trainer (ctgcn_amd/embedding.py): batch partition, epoch order, sample seeds, export file names."""
import pytest
import torch


def test_batch_partition_and_count():
    from ctgcn_amd.embedding import batch_bounds, batch_count
    assert batch_count(1_000_000, 2048) == 489                   # config 5 under the shipped batch_size
    assert batch_count(4096, 2048) == 2 and batch_count(1, 2048) == 1
    b = batch_bounds(1100, 256)
    assert b == [(0, 256), (256, 512), (512, 768), (768, 1024), (1024, 1100)]
    assert batch_bounds(512, 256) == [(0, 256), (256, 512)]


def test_epoch_order_is_the_reference_randperm():
    from ctgcn_amd.embedding import epoch_order
    torch.manual_seed(42)
    want = [torch.randperm(1000) for _ in range(3)]               # reference embedding.py:340, one draw per epoch
    torch.manual_seed(42)
    got = [epoch_order(1000) for _ in range(3)]
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert torch.equal(epoch_order(7, shuffle=False), torch.arange(7))


def test_sample_seed_derivation():
    from ctgcn_amd.metrics import epoch_batch_seed
    s = epoch_batch_seed(5, 0, 0, 0)
    assert s == epoch_batch_seed(5, 0, 0, 0) and 0 <= s < 2 ** 64
    seeds = {epoch_batch_seed(5, e, b, t) for e in range(4) for b in range(20) for t in range(3)}
    assert len(seeds) == 4 * 20 * 3                                  # every (epoch, batch, snapshot) draws its own stream
    assert epoch_batch_seed(6, 0, 0, 0) != s
    assert epoch_batch_seed(5, 1, 0, 0) != epoch_batch_seed(5, 0, 1, 0) != epoch_batch_seed(5, 0, 0, 1)
    assert epoch_batch_seed(2 ** 64 + 5, 0, 0, 0) == s               # a 64-bit stream


def test_timestamp_to_file_name():
    from ctgcn_amd.embedding import snapshot_file_stem
    stamps = sorted(["2004-05.csv", "2004-04.csv", "2004-06.txt"])
    assert [snapshot_file_stem(stamps, 1, i) for i in range(2)] == ["2004-05", "2004-06"]
    assert snapshot_file_stem(["a.b.csv"], 0, 0) == "a"                # reference: split('.')[0]


def test_cpu_trainer_is_refused(tmp_path):
    from ctgcn_amd import CTGCN, ReconstructionLoss
    from ctgcn_amd._lib import CtgcnHipError
    from ctgcn_amd.embedding import UnsupervisedEmbedding
    (tmp_path / "origin").mkdir()
    with pytest.raises(CtgcnHipError):
        UnsupervisedEmbedding(str(tmp_path), "origin", "emb", ["a"], CTGCN(4, 8, 8, 1, 1, 1, model_type="S"), ReconstructionLoss())
