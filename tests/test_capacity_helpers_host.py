"""CPU: the two helpers every capacity-mode loop shares -- ``node_capacity`` (round N up to the bucket, at most B * T) and
``trainer.batch_table`` (the int32 [steps, 2 B] table of an epoch), the latter against the two constructions it replaced."""
import numpy as np
import torch


def test_node_capacity_rounds_up_to_the_bucket_at_most_b_times_t():
    from erc_amd.capacity import node_capacity
    from erc_amd import trainer
    assert trainer.node_capacity is node_capacity
    assert [node_capacity(n, 128, 4 * 70) for n in (0, 1, 128, 129)] == [0, 128, 128, 256]
    assert node_capacity(257, 128, 4 * 70) == 280                       # clipped to B * T
    assert [node_capacity(n, 128, 2 * 7) for n in (0, 1, 13, 14)] == [0, 14, 14, 14]      # B * T below one bucket
    assert node_capacity(257, 256, 4 * 70) == 280 and node_capacity(256, 256, 4 * 70) == 256


def test_batch_table_equals_the_two_constructions_it_replaced():
    from erc_amd.trainer import batch_table
    lengths = [40, 3, 50, 7, 1, 60, 60, 60, 22, 2]
    B, n = 4, len(lengths)
    steps = -(-n // B)
    lens = np.asarray(lengths, dtype=np.int32)
    offs = (np.cumsum([0] + lengths)[:-1]).astype(np.int32)
    order = torch.randperm(n, generator=torch.Generator().manual_seed(3)).numpy()
    # ResidentEpochs.plan as it was: two flat arrays, reshaped into the halves of a preallocated table
    flat_l, flat_o = np.zeros(steps * B, dtype=np.int32), np.zeros(steps * B, dtype=np.int32)
    flat_l[:n], flat_o[:n] = lens[order], offs[order]
    want = np.zeros((steps, 2 * B), dtype=np.int32)
    want[:, :B], want[:, B:] = flat_l.reshape(steps, B), flat_o.reshape(steps, B)
    got = batch_table(lens, offs, order, B)
    assert got.dtype == np.int32 and got.shape == (steps, 2 * B) and np.array_equal(got, want)
    # ResidentEval.__init__ as it was: the store's own order, the halves concatenated
    flat_l[:n], flat_o[:n] = lens, offs
    want = np.concatenate([flat_l.reshape(steps, B), flat_o.reshape(steps, B)], axis=1)
    assert np.array_equal(batch_table(lens, offs, np.arange(n), B), want)
    assert want[-1].tolist() == [22, 2, 0, 0, int(offs[8]), int(offs[9]), 0, 0]      # zeros in the last batch's empty slots


def test_zero_row_stores_keep_one_extension_per_store():
    """one tensor or a dict of them, a zero row appended; the same object for the same store, another for another store, and
    both still there when the two alternate (a run's train and test store)"""
    import types
    from erc_amd.capacity import ZeroRowStores
    ext = ZeroRowStores()
    train = types.SimpleNamespace(fused=torch.ones(10, 6, dtype=torch.bfloat16))
    test = types.SimpleNamespace(fused=torch.ones(4, 6, dtype=torch.bfloat16))
    a, b = ext(train, train.fused), ext(test, test.fused)
    assert a.shape == (11, 6) and a.dtype == torch.bfloat16 and torch.equal(a[:10], train.fused) and float(a[10].abs().sum()) == 0
    assert b.shape == (5, 6) and torch.equal(b[:4], test.fused) and float(b[4].abs().sum()) == 0
    assert a is not b
    for _ in range(2):                                                    # alternating stores: nothing is rebuilt
        assert ext(train, train.fused) is a and ext(test, test.fused) is b
    # identity, not equality: a store that merely looks the same gets an extension of its own
    twin = types.SimpleNamespace(fused=train.fused)
    assert ext(twin, twin.fused) is not a and ext(train, train.fused) is a
    # a dict of tensors (one per modality): every entry extended, the dict itself cached
    mm = types.SimpleNamespace(feats=dict(a=torch.ones(3, 2), v=torch.ones(3, 5, dtype=torch.float64)))
    d = ext(mm, mm.feats)
    assert set(d) == {"a", "v"} and d["a"].shape == (4, 2) and d["v"].shape == (4, 5) and d["v"].dtype == torch.float64
    assert all(torch.equal(d[m][:3], mm.feats[m]) and float(d[m][3].abs().sum()) == 0 for m in d)
    assert ext(mm, mm.feats) is d and ext(train, train.fused) is a
