"""GPU: the graph slices of the COGMEN tile kernels in their two forms (erc_set_tile_slices / ERC_TILE_SLICES): ``csr`` loads
in_ptr / in_src / in_typ / out_ptr / out_dst / out_typ / inv_cnt, ``closed`` derives the same integers from the node records
the projection launch writes (position in the dialogue, dialogue length, first in-edge, first out-edge) and the speakers.
Same integers, hence the same bits: every output of the forward tile, the head and the backward tile launches is compared
with torch.equal on the raw bytes.

The feature block has 16 feature columns; the projection launch takes K >= 32 (erc_cogmen_project_graph_ok), so the block
carries 16 zero columns behind them (K = 32).  A narrower block would send the step down the separate graph-build launch,
which writes no records: both forms would read the CSR and the comparison would be empty -- every run below asserts that the
records were there."""
import types

import pytest
import torch

from erc_amd import capi
from erc_amd import cogmen as cg
from tests.util_cases import cogmen_case_lengths

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DIMS16 = dict(a=4, t=8, v=4)              # D = 16 features ...
K_PAD = 32                                # ... in a block of 32 columns (the projection launch's smallest K)
F = 100
# tiles of 16 rows begin and end inside, at and across dialogue boundaries; dialogues shorter than the window (N = 98: 7 tiles)
LENGTHS = (1, 2, 6, 11, 12, 16, 17, 33)
ORDERS = {"asc": LENGTHS, "desc": LENGTHS[::-1]}
WINDOWS = [(5, 5), (0, 0), (5, 0), (0, 5), (1, 3)]
SPEAKERS = ("alternating", "all0", "all1", "random")
FORMS = ("csr", "closed")


@pytest.fixture(autouse=True)
def _default_form_afterwards():
    yield
    capi.set_tile_slices(True)


@pytest.fixture
def window(monkeypatch):
    def set_window(wp, wf):
        monkeypatch.setattr(cg, "WP", wp)
        monkeypatch.setattr(cg, "WF", wf)
    return set_window


def _bytes(t):
    return t.contiguous().reshape(-1).view(torch.uint8)


def _same_bits(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bytes(a), _bytes(b)), what


def _speakers(pattern, B, T):
    if pattern == "alternating":
        return (torch.arange(T) % 2).repeat(B, 1)
    if pattern == "all0":
        return torch.zeros(B, T, dtype=torch.int64)
    if pattern == "all1":
        return torch.ones(B, T, dtype=torch.int64)
    return torch.randint(0, 2, (B, T), generator=torch.Generator().manual_seed(7))


def _batch(lengths, pattern):
    b = dict(cogmen_case_lengths(lengths, dims=DIMS16, seed=3)["batch"])
    x = b["input_tensor"]
    assert x.shape[2] == 16
    b["input_tensor"] = torch.cat([x, x.new_zeros(x.shape[0], x.shape[1], K_PAD - 16)], dim=2).contiguous()
    b["speaker_tensor"] = _speakers(pattern, x.shape[0], x.shape[1]).to(b["speaker_tensor"].dtype)
    return b


def _trainer(compute, D=K_PAD):
    from erc_amd.params import ERCParams
    torch.manual_seed(0)
    p = ERCParams().from_args(["--dataset=iemocap-cogmen-sbert-6", "--compute=" + compute, "--train.batch_size=8"])
    p.hidden_all = D
    return cg.COGMENTrainer(p, DEV)


def _expected_records(g, lengths, N):
    """records recomputed on the host from in_ptr / out_ptr and the lengths (node order = dialogue order); record N = (0, 0, E, E)"""
    in_ptr, out_ptr = g["in_ptr"][:N + 1].cpu(), g["out_ptr"][:N + 1].cpu()
    pos = torch.cat([torch.arange(int(L)) for L in lengths] + [torch.zeros(1, dtype=torch.int64)])
    length = torch.cat([torch.full((int(L), ), int(L)) for L in lengths] + [torch.zeros(1, dtype=torch.int64)])
    return torch.stack([pos, length, in_ptr.long(), out_ptr.long()], dim=1).to(torch.int32)


def _outputs(tr, ws, N, stats):
    """every output of the forward tile, head and backward tile launches (rows < N), the step's gradients and state"""
    torch.cuda.synchronize()
    g, fp = ws["g"], tr.model.flat
    assert g.get("node_rec") is not None, "the step did not go through the projection + graph launch: no records"
    E, tiles = int(g["in_ptr"][N]), -(-N // 16)
    split = tr.model.terms > 1
    rows = (dict(M=900, H1=100, dQKVS=400, dH1=100, dH0=100) if split else dict(Mb=900, H1b=100, dQKVSb=400, dH1b=100, dH0b=100))
    rows.update(QKVS=400, H2=100, inv_cnt=8, logits=6)
    out = {k: ws[k][:N, :c].clone() for k, c in rows.items()}
    out["alpha"] = ws["alpha"][:E].clone()
    out["bn_partials"] = ws["bn_tile_ws"].view(torch.float32)[4:4 + tiles * 2 * F].clone()
    out["bn_saved"] = ws["bn_saved"].clone()
    out["dgamma"], out["dbeta"] = fp.g("gcn.bn.weight").clone(), fp.g("gcn.bn.bias").clone()
    out["stats"] = stats.detach().clone()
    out.update({"data": fp.data.clone(), "exp_avg": fp.exp_avg.clone(), "exp_avg_sq": fp.exp_avg_sq.clone(), "grad_full": fp.grad_full.clone()})
    out.update({k: v.detach().clone() for k, v in tr.model.state_dict().items() if "running_" in k})
    assert ws["bn_in_tile"] and ws["head_deferred"]                  # forward tile sums -> head -> backward tile adds the head's records
    assert float(out["QKVS"].abs().max()) > 0 and float(out["alpha"].abs().max()) > 0 and E >= N
    assert float(out["dgamma"].abs().max()) > 0
    gk = "dH0" if split else "dH0b"
    assert float(out[gk].float().abs().max()) > 0
    return out


def _exact_step(form, compute, lengths, pattern):
    capi.set_tile_slices(form == "closed")
    tr = _trainer(compute)
    batch = tr.prepare_batch(_batch(lengths, pattern))
    x = batch["input_tensor"]
    B, T, N = x.shape[0], x.shape[1], int(batch["label"].shape[0])
    ws = tr.model._workspace(B, T, N, x.device)
    stats = tr.train_step(batch)
    assert tr.model._last_ws is ws
    out = _outputs(tr, ws, N, stats)
    out["node_rec"] = ws["g"]["node_rec"][:N + 1].clone()
    assert torch.equal(out["node_rec"].cpu(), _expected_records(ws["g"], lengths, N)), "node records"
    return out


def _compare(runs):
    a, b = runs["csr"], runs["closed"]
    assert a.keys() == b.keys()
    for k in a:
        _same_bits(a[k], b[k], k)


@pytest.mark.parametrize("order", list(ORDERS))
@pytest.mark.parametrize("wp,wf", WINDOWS)
@pytest.mark.parametrize("compute", ["bf16", "f32x3"], ids=["bf16-block", "fp32-block"])
def test_csr_and_closed_form_give_the_same_bits(window, compute, wp, wf, order):
    """one eager training step per form and speaker pattern: projection + graph + records, forward tile, head, backward tile
    (and the weight-gradient + Adam launch behind them: equal inputs, equal parameters and moments)"""
    window(wp, wf)
    for pattern in SPEAKERS:
        _compare({form: _exact_step(form, compute, ORDERS[order], pattern) for form in FORMS})


def test_two_term_compute_mode(window):
    """(bf16 and f32x3 are the two cases of the grid above)"""
    window(5, 5)
    _compare({form: _exact_step(form, "f32x2", LENGTHS, "random") for form in FORMS})


@pytest.mark.parametrize("wp,wf", WINDOWS)
@pytest.mark.parametrize("pattern", SPEAKERS)
def test_node_records_of_the_projection_launch(window, pattern, wp, wf):
    """the records alone, both dialogue orders, against the host's recomputation -- integer equality"""
    window(wp, wf)
    tr = _trainer("bf16")
    for order in ORDERS:
        batch = tr.prepare_batch(_batch(ORDERS[order], pattern))
        x = batch["input_tensor"]
        B, T, N = x.shape[0], x.shape[1], int(batch["label"].shape[0])
        m = tr.model
        ws = m._workspace(B, T, N, x.device)
        ws["g"]["node_rec"] = ws["node_rec"]
        ws["node_rec"].fill_(-7)
        capi.cogmen_project_graph(x, K_PAD, m.w1_shadow, K_PAD, m.flat.w("rnn.1.bias"), ws["H0"], F, F, K_PAD, batch["text_length"],
                                  batch["speaker_tensor"], B, T, wp, wf, 2, N, ws["E"], ws["g"])
        torch.cuda.synchronize()
        assert torch.equal(ws["node_rec"].cpu(), _expected_records(ws["g"], ORDERS[order], N))
        # the closed forms the tile kernels evaluate, against the CSR itself
        rec, g = ws["node_rec"][:N].cpu().long(), {k: v.cpu().long() for k, v in ws["g"].items() if v is not None}
        node = torch.arange(N)
        assert torch.equal(g["in_src"][rec[:, 2]], node - torch.minimum(rec[:, 0], torch.tensor(wf)))          # first source
        assert torch.equal(g["out_dst"][rec[:, 3]], node - torch.minimum(rec[:, 0], torch.tensor(wp)))         # first target
        deg_in = torch.minimum(rec[:, 1] - 1, rec[:, 0] + wp) - (rec[:, 0] - wf).clamp(min=0) + 1
        deg_out = torch.minimum(rec[:, 1] - 1, rec[:, 0] + wf) - (rec[:, 0] - wp).clamp(min=0) + 1
        assert torch.equal(g["in_ptr"][1:N + 1] - g["in_ptr"][:N], deg_in)
        assert torch.equal(g["out_ptr"][1:N + 1] - g["out_ptr"][:N], deg_out)


# -------------------------------------------------------------------------------------------------- capacity and resident forms
def _capacity_step(form, compute, pattern):
    """the batch in the static buffers of its capacity bucket: N_cap = 256 rows for N = 98, the node count read on the device"""
    capi.set_tile_slices(form == "closed")
    tr = _trainer(compute)
    batch = tr.prepare_batch(_batch(LENGTHS, pattern))
    N = int(batch["label"].shape[0])
    tr.t_cap = 40
    key, make, fill = tr.capacity_bucket(batch)
    assert key == ("capacity", 8, 40, 256) and N < 256
    static = make()
    fill(static, batch)
    tr.model.dynamic_n = True
    try:
        stats = tr.train_step(static)
    finally:
        tr.model.dynamic_n = False
    ws = tr.model._last_ws
    out = _outputs(tr, ws, N, stats)
    assert int(ws["g"]["counts"][0]) == N
    assert torch.equal(ws["g"]["node_rec"][:N + 1].cpu(), _expected_records(ws["g"], LENGTHS, N)), "node records (capacity form)"
    return out


def _resident_step(form, compute, pattern):
    """the dialogues in a feature store, the batch a list of dialogue slots (desc): one empty slot, slots not in store order"""
    capi.set_tile_slices(form == "closed")
    tr = _trainer(compute)
    b = tr.prepare_batch(_batch(LENGTHS, pattern))
    lens = [int(v) for v in b["text_length"]]
    x, spk = b["input_tensor"], b["speaker_tensor"]
    store_order = [3, 0, 7, 1, 5, 2, 6, 4]                           # dialogue i of the batch sits at position store_order.index(i)
    starts, rows, lab, lab_off = {}, [], [], [0]
    for L in lens:
        lab_off.append(lab_off[-1] + L)
    at = 0
    for i in store_order:
        starts[i] = at
        rows.append((x[i, :lens[i]], spk[i, :lens[i]], b["label"][lab_off[i]:lab_off[i + 1]]))
        at += lens[i]
    store = types.SimpleNamespace(fused=torch.cat([r[0] for r in rows]).contiguous(), speaker=torch.cat([r[1] for r in rows]).contiguous(),
                                  label=torch.cat([r[2] for r in rows]).contiguous())
    slots = [0, 1, 2, None, 3, 4, 5, 6, 7]                           # slot 3 is empty
    desc = torch.tensor([lens[i] if i is not None else 0 for i in slots] + [starts[i] if i is not None else 0 for i in slots],
                        dtype=torch.int32, device=DEV)
    N = sum(lens)
    batch = tr.resident_batch(store, desc, len(slots), 40, 128)
    assert batch is not None and N < 128
    tr.model.dynamic_n = True
    try:
        stats = tr.train_step(batch)
    finally:
        tr.model.dynamic_n = False
    ws = tr.model._last_ws
    out = _outputs(tr, ws, N, stats)
    assert int(ws["g"]["counts"][0]) == N
    assert torch.equal(ws["g"]["node_rec"][:N + 1].cpu(), _expected_records(ws["g"], LENGTHS, N)), "node records (resident form)"
    return out


@pytest.mark.parametrize("compute", ["bf16", "f32x3"])
def test_capacity_form(window, compute):
    window(5, 5)
    _compare({form: _capacity_step(form, compute, "random") for form in FORMS})


@pytest.mark.parametrize("compute", ["bf16", "f32x3"])
def test_resident_form(window, compute):
    window(5, 5)
    _compare({form: _resident_step(form, compute, "random") for form in FORMS})


# -------------------------------------------------------------------------------------------------- replayed steps
def _replayed(monkeypatch, form, compute, replays=3):
    from erc_amd.engine import GraphedStep
    monkeypatch.setenv("ERC_TILE_SLICES", form)
    tr = _trainer(compute, D=48)
    batch = tr.prepare_batch(cogmen_case_lengths((20, 7, 13, 1), dims=dict(a=12, t=20, v=16), seed=3)["batch"])     # B = 4, T = 20
    assert tuple(batch["input_tensor"].shape[:2]) == (4, 20)
    step = GraphedStep(lambda: tr.train_step(batch))
    assert step.captured.slices == form
    for _ in range(replays):
        stats = step()
    torch.cuda.synchronize()
    assert tr.model._last_ws["g"].get("node_rec") is not None
    fp = tr.model.flat
    out = {"data": fp.data, "exp_avg": fp.exp_avg, "exp_avg_sq": fp.exp_avg_sq, "stats": stats}
    out.update({k: v for k, v in tr.model.state_dict().items() if "running_" in k})
    return {k: v.detach().clone() for k, v in out.items()}


@pytest.mark.parametrize("compute", ["bf16", "f32x32"])
def test_three_replayed_steps(monkeypatch, compute):
    runs = {form: _replayed(monkeypatch, form, compute) for form in FORMS}
    _compare(runs)
    assert float(runs["csr"]["exp_avg"].abs().max()) > 0


def test_unknown_form_is_refused_by_the_library():
    with pytest.raises(capi.ErcGraftError, match="set_tile_slices"):
        capi._call("erc_set_tile_slices", 2)
