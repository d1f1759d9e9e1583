"""CPU: erc_chain_order (csrc/launch_chain.hip) -- the host function that decides whether the edges of a captured graph
form one simple path, and in which order its kernel nodes run.  hipGraphGetNodes promises no order, so the order must come
from the edges alone."""
import pytest

from erc_amd import capi


def test_a_path_given_in_shuffled_node_order():
    # the path 3 -> 0 -> 4 -> 1 -> 2, its edges listed in no particular order
    assert capi.chain_order(5, [(4, 1), (3, 0), (1, 2), (0, 4)]) == [3, 0, 4, 1, 2]
    assert capi.chain_order(2, [(1, 0)]) == [1, 0]
    assert capi.chain_order(4, [(0, 1), (1, 2), (2, 3)]) == [0, 1, 2, 3]


def test_a_single_node_is_a_path():
    assert capi.chain_order(1, []) == [0]


@pytest.mark.parametrize("n, edges, what", [
    (3, [(0, 2)], "two roots"),                                  # 0 -> 2 and a lone node 1
    (4, [(0, 1), (2, 3), (3, 2)], "two roots / cycle"),          # right edge count, a 2-cycle beside a path
    (3, [(0, 1), (0, 2)], "fork"),
    (4, [(0, 1), (0, 2), (1, 3)], "fork"),
    (3, [(0, 2), (1, 2)], "join"),
    (4, [(0, 1), (0, 2), (1, 3), (2, 3)], "fork and join"),      # what a capture forked over two streams looks like
    (3, [(0, 1), (1, 2), (1, 2)], "duplicate edge"),
    (3, [(0, 1), (0, 1)], "duplicate edge with the right count"),
    (3, [(0, 1), (1, 2), (2, 0)], "cycle"),
    (2, [(0, 0)], "self edge"),
    (2, [(0, 2)], "index out of range"),
    (2, [(-1, 1)], "negative index"),
    (0, [], "n = 0"),
    (-1, [], "n < 0"),
])
def test_anything_but_one_simple_path_is_refused(n, edges, what):
    with pytest.raises(capi.ErcGraftError, match="erc_chain_order.*chain_order"):
        capi.chain_order(n, edges)


def test_not_a_chain_handle_is_reported_not_followed():
    capi.chain_free(0)                                           # null is accepted
    with pytest.raises(capi.ErcGraftError, match="chain_len"):
        capi.chain_len(0)
    handle, why = capi.chain_build(None)                         # no graph: refused with a reason, not followed
    assert handle == 0 and "chain_build" in why
