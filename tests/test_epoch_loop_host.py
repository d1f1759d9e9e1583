"""CPU: ``trainer.EpochLoop`` with a stub trainer on ``torch.device("cpu")`` -- which batches an epoch visits, in which order,
what it returns and where a step's stats go.  No kernel runs here: there is no GPU."""
import functools

import pytest
import torch

from erc_amd import trainer as T
from erc_amd.collate import ERCCollate
from erc_amd.params import ERCParams

ARGV = ["--graph_replay=False", "--n_train=10", "--n_test=5", "--train.batch_size=4", "--test.batch_size=4", "--syn_min_len=1",
        "--syn_max_len=9"]
CPU = torch.device("cpu")


def _params(extra=()):
    return ERCParams().from_args(ARGV + list(extra))


def _prints(batch):
    """one fingerprint per dialogue of a collated batch: its length and the bytes of its first feature row"""
    x, lens = batch["input_tensor"], batch["text_length"].tolist()
    x = x if _params().batch_first else x.transpose(0, 1)
    return tuple((n, x[b, 0].numpy().tobytes()) for b, n in enumerate(lens))


@functools.lru_cache(maxsize=None)
def _split():
    """(fingerprints of the training dialogues, #training utterances, the test labels in order)"""
    p = _params()
    train, test = T.load_dialogues(p)
    collate = ERCCollate(p)
    return (frozenset(_prints(collate([[d]]))[0] for d in train), sum(len(d["label"]) for d in train),
            tuple(int(v) for d in test for v in d["label"]))


class _Model:
    def train(self):
        pass

    def eval(self):
        pass


class _Stub:
    """records the batches it is given; step ``i`` of its life returns the stats [i, #utterances, 0.5, 0.25]"""

    def __init__(self):
        self.model, self.seen, self.steps = _Model(), [], 0

    def prepare_batch(self, batch):
        return batch

    def train_step(self, batch):
        self.seen.append(_prints(batch))
        self.steps += 1
        return torch.tensor([self.steps - 1, int(batch["label"].shape[0]), 0.5, 0.25])

    def to_logits(self, batch):
        return torch.zeros(int(batch["label"].shape[0]), 6)


def _loop(extra=()):
    p = _params(extra)
    T.fix_seed(p.seed)
    tr = _Stub()
    return T.EpochLoop(p, tr, CPU), tr


def test_a_loader_epoch_visits_every_dialogue_once_and_fills_the_ring():
    prints, n_utt, _ = _split()
    loop, tr = _loop()
    assert loop.counters is None and loop.graphs is None and loop.fixed is None and loop.resident is None and loop.res_eval is None
    assert loop.n_steps == 3 and tuple(loop.ring.shape) == (3, 4)
    orders = []
    for epoch in range(2):
        tr.seen = []
        got, counts = loop.train_epoch()
        flat = [d for b in tr.seen for d in b]
        assert len(flat) == 10 and frozenset(flat) == prints and len(prints) == 10      # every dialogue exactly once
        assert [len(b) for b in tr.seen] == [4, 4, 2]                                      # the smaller last batch
        assert counts == [sum(n for n, _ in b) for b in tr.seen] and sum(counts) == got == n_utt
        assert loop.ring.tolist() == [[3.0 * epoch + i, float(c), 0.5, 0.25] for i, c in enumerate(counts)]
        orders.append(flat)
    assert orders[0] != orders[1]
    again, tr2 = _loop()
    for want in orders:                                                                  # same seed: the same epochs again
        tr2.seen = []
        again.train_epoch()
        assert [d for b in tr2.seen for d in b] == want


def test_a_test_epoch_returns_the_test_splits_labels_in_order():
    _, _, labels = _split()
    loop, _ = _loop()
    res = loop.test_epoch()
    assert res.cm is None and tuple(res.true) == labels and res.pred == [0] * len(labels)
    assert res.true_multi == [] and res.prob_multi == []


def test_fixed_batches_are_the_same_collated_batches_in_a_reshuffled_order():
    prints, n_utt, _ = _split()
    loop, tr = _loop(["--fixed_batches"])
    assert loop.counters is None and len(loop.fixed) == loop.n_steps == 3
    tr.seen, epochs = [], []
    for _ in range(4):
        tr.seen = []
        got, counts = loop.train_epoch()
        assert got == n_utt and counts == [sum(n for n, _ in b) for b in tr.seen]
        epochs.append(list(tr.seen))
    assert frozenset(d for b in epochs[0] for d in b) == prints
    assert all(sorted(e) == sorted(epochs[0]) for e in epochs[1:])      # the very same batches ...
    assert any(e != epochs[0] for e in epochs[1:])                       # ... visited in another order


def test_resident_without_device_collate_exits_before_the_first_epoch():
    with pytest.raises(SystemExit) as exc:
        _loop(["--resident"])
    assert str(exc.value) == "--resident needs --device_collate, one rank and a trainer with resident batches (capacity mode)"


def test_resident_loops_on_a_dialogue_store_take_two_ints_per_slot_and_the_stores_longest_dialogue():
    """the descriptor width and T are the store's (``DESC_INTS``, ``t_max``): a DeviceDialogueStore gives 2 B int32 and its
    longest dialogue, MMIN's utterance store 3 B (tests/test_mmin_cap_ref.py)"""
    from erc_amd.datasets import DeviceDialogueStore, MMINDeviceStore
    p = _params()
    train, test = T.load_dialogues(p)
    assert (DeviceDialogueStore.DESC_INTS, MMINDeviceStore.DESC_INTS) == (2, 3)
    for dialogs, B in ((train, 4), (test, 3)):
        store = DeviceDialogueStore(dialogs, p, CPU)
        longest = max(len(d["label"]) for d in dialogs)
        assert store.t_max == longest == int(store.lengths.max())
        for loop in (T.ResidentEpochs(_Stub(), store, B, seed=3), T.ResidentEval(_Stub(), store, B, n_classes=6)):
            assert loop.cur_desc.shape == (2 * B, ) and loop.cur_desc.dtype == torch.int32
            assert loop.T == longest and loop.B == B and loop.graphs == {}
            loop.drop_graphs()                                          # nothing captured yet: nothing to drop
            assert loop.graphs == {}
