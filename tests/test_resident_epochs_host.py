"""CPU: ``trainer.ResidentEpochs`` (``--resident``) under a recorder in place of the HIP runtime (its ``_capture`` seam): the
planned permutations, the batch tables, the descriptor copy per step, one eager step + one capture per node capacity and a
replay for everything else, the dynamic-N switch, ``capture=False`` and what ``supported()`` probes."""
import types

import pytest
import torch

LENGTHS = [40, 3, 50, 7, 1, 60, 60, 60, 22, 2]                          # n = 10, B = 4 -> 3 steps, the last with 2 dialogues
B = 4


class _Store:
    DESC_INTS = 2

    def __init__(self, lengths):
        self.lengths = torch.tensor(lengths, dtype=torch.int64)
        self.t_max = max(lengths)
        self.offsets = torch.zeros(len(lengths) + 1, dtype=torch.int64)
        self.offsets[1:] = torch.cumsum(self.lengths, 0)
        self.device = "cpu"

    def __len__(self):
        return int(self.lengths.numel())


class _Trainer:
    """what ResidentEpochs asks of a trainer: ``resident_batch``, ``train_step`` and a model with ``dynamic_n``"""

    def __init__(self, refuse_above=None, fail_at=None):
        self.model = types.SimpleNamespace(dynamic_n=False, _last_ws={"ws": 0})
        self.refuse_above, self.fail_at = refuse_above, fail_at
        self.asked, self.steps, self.flags = [], [], []

    def resident_batch(self, store, cur_desc, B_cap, T_cap, N_cap):
        self.asked.append((B_cap, T_cap, N_cap))
        if self.refuse_above is not None and N_cap > self.refuse_above:
            return None
        return dict(desc=cur_desc, caps=(B_cap, T_cap, N_cap))

    def train_step(self, batch):
        self.flags.append(self.model.dynamic_n)
        if self.fail_at is not None and len(self.steps) == self.fail_at:
            raise RuntimeError("step failed")
        self.steps.append((batch["caps"], batch["desc"].tolist()))
        self.model._last_ws = {"ws": batch["caps"][2]}
        n = float(batch["desc"][:batch["caps"][0]].sum())
        return torch.tensor([2.0 * n, n, 1.0, 0.0, 9.0])


def _resident(tr, calls, seed=11, capture=True):
    """a capture records and does not execute, like the real one; a replay notes the descriptor it would run on"""
    from erc_amd.trainer import ResidentEpochs
    res = ResidentEpochs(tr, _Store(LENGTHS), B, seed, capture=capture)
    res._capture = lambda fn: types.SimpleNamespace(
        replay=lambda: calls.append(("replay", res.cur_desc.tolist(), tr.model.dynamic_n)))
    return res


def _tables(res):
    return [t.clone() for _, _, t in res._ahead]


def test_plan_ahead_draws_the_permutations_of_separate_plans():
    a, b = _resident(_Trainer(), []), _resident(_Trainer(), [])
    a.plan(2)
    ta = _tables(a)
    tb = []
    for _ in range(2):
        b.plan(1)
        tb += _tables(b)
        b.epoch()
    assert len(ta) == 2 and all(torch.equal(x, y) for x, y in zip(ta, tb))
    assert not torch.equal(ta[0], ta[1])                                 # two different permutations
    assert a.epoch() == (sum(LENGTHS), 3) and a.epoch() == (sum(LENGTHS), 3) and a._ahead == []
    assert a.epoch() == (sum(LENGTHS), 3)                                # an epoch nobody planned plans itself


def test_table_rows_hold_lengths_then_first_rows_with_zero_padding():
    res = _resident(_Trainer(), [])
    res.plan(1)
    tab = _tables(res)[0]
    assert tab.shape == (3, 2 * B) and tab.dtype == torch.int32
    offs = res.store.offsets[:-1].tolist()
    order = torch.randperm(len(LENGTHS), generator=torch.Generator().manual_seed(11)).tolist()
    for s in range(3):
        ids = order[B * s:B * s + B]
        pad = [0] * (B - len(ids))
        assert tab[s, :B].tolist() == [LENGTHS[i] for i in ids] + pad
        assert tab[s, B:].tolist() == [offs[i] for i in ids] + pad
    assert len(order[2 * B:]) == 2                                       # the last batch is the smaller one


def test_each_capacity_runs_eagerly_once_is_captured_once_and_then_replays():
    tr, calls = _Trainer(), []
    res = _resident(tr, calls)
    assert res.N_BUCKET == 128 and res.T == 60 and res.cur_desc.shape == (2 * B, ) and res.cur_desc.dtype == torch.int32
    res.plan(2)
    tabs = _tables(res)
    rows = [t[s].tolist() for t in tabs for s in range(3)]
    caps = [min(-(-sum(r[:B]) // 128) * 128, B * 60) for r in rows]
    assert len(set(caps)) > 1                                            # more than one capacity in these two epochs
    n_utt = [res.epoch()[0], res.epoch()[0]]
    assert n_utt == [sum(LENGTHS)] * 2
    # every step ran on its own row: eager steps saw it in the descriptor, replays found it there
    first = {c: caps.index(c) for c in set(caps)}
    want_eager = [((B, 60, c), rows[i]) for c, i in sorted(first.items(), key=lambda kv: kv[1])]
    assert tr.steps == want_eager
    assert [c[1] for c in calls] == [rows[i] for i in range(6) if i not in first.values()]
    assert (res.eager, res.captures, res.replays) == (len(first), len(first), 6 - len(first))
    assert res.replays + res.eager == 6
    assert sorted(res.graphs) == sorted(first) and all(res.graphs[c][2] == {"ws": c} for c in first)      # workspace kept
    assert res.acc.tolist()[:2] == [2.0 * sum(sum(r[:B]) for _, r in tr.steps), sum(sum(r[:B]) for _, r in tr.steps)]
    # capacity mode inside every step, off again afterwards
    assert tr.flags == [True] * len(first) and all(c[2] for c in calls) and tr.model.dynamic_n is False


def test_dynamic_n_is_off_again_when_a_step_raises():
    tr = _Trainer(fail_at=0)
    res = _resident(tr, [])
    with pytest.raises(RuntimeError, match="step failed"):
        res.epoch()
    assert tr.flags == [True] and tr.model.dynamic_n is False


def test_without_capture_every_step_stays_eager():
    tr, calls = _Trainer(), []
    res = _resident(tr, calls, capture=False)
    res.epoch()
    res.epoch()
    assert (res.eager, res.captures, res.replays) == (6, 0, 0) and calls == [] and len(tr.steps) == 6
    assert tr.flags == [True] * 6 and tr.model.dynamic_n is False


def test_supported_probes_the_smallest_and_the_worst_case_capacity():
    tr = _Trainer()
    res = _resident(tr, [])
    assert res.supported()
    assert tr.asked == [(B, 60, 128), (B, 60, 240)]                      # 4 x 60 = 240 nodes -> 256, at most B * T = 240
    assert not _resident(_Trainer(refuse_above=128), []).supported()
    assert _resident(_Trainer(refuse_above=240), []).supported()
    small = _Trainer()
    from erc_amd.trainer import ResidentEpochs
    assert ResidentEpochs(small, _Store([5, 6, 7]), 2, 0).supported() and small.asked == [(2, 7, 128)]      # never below one bucket
