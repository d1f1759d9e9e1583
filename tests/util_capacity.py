"""CPU: what the capacity-bucket host tests of several trainers share."""
import torch

# (B, T) of the batches: both shrink, both grow, one grows while the other shrinks, and each moves alone in each direction
FILL_SEQ = ([9, 8, 10, 7], [3, 4], [12, 12, 12, 11], [1], [2, 11], [5, 5, 5, 5], [12, 1], [12, 3, 3], [4, 4, 4], [4, 4], [7, 2])


def assert_fill_equals_a_fresh_buffer(tr, batches, first_key):
    """after every fill of one static dict, each of its entries equals make() + fill of that batch alone"""
    key, make, fill = tr.capacity_bucket(batches[0])
    assert key == ("capacity", 4, 12, 48)
    static = make()
    for i, b in enumerate(batches):
        assert tr.capacity_bucket(b)[0] == key
        fill(static, b)
        fresh = make()
        fill(fresh, b)
        assert set(static) == set(fresh)
        for k, v in fresh.items():
            assert torch.equal(static[k], v) if torch.is_tensor(v) else static[k] == v, (i, k)
        r, c = b[first_key].shape[:2]
        assert torch.equal(static[first_key][:r, :c], b[first_key]), i          # (and the batch itself is in there)
        rest = static[first_key].clone()
        rest[:r, :c] = 0
        assert int(rest.count_nonzero()) == 0, i                                  # (and nothing else)
