"""CPU: COGMEN's capacity buckets (COGMENTrainer.capacity_bucket / all_capacity_buckets / resident_batch) -- keys and
rounding at N_BUCKET = 256, a bucket-shaped batch still getting a bucket, the refusals, the precapture list without a clipped
top entry, the synthetic lengths, and the resident batch's refusals.

``COGMENTrainer(params, "cpu")`` cannot be built without a GPU in the bf16 mode these buckets belong to: its constructor
refreshes the bf16 weight shadows with a device kernel.  The trainer is therefore stood up with ``object.__new__`` plus the
attributes these methods read (params, device, encoder, model); the model is a namespace carrying the fields of the fused bf16
path, with COGMENModule's own ``supports_capacity`` and ``BN_FUSED_MAX_N``."""
import types

import torch

D = 100


def _trainer(batch_size=4, t_cap=70, terms=1):
    from erc_amd.cogmen import COGMENModule, COGMENTrainer
    tr = object.__new__(COGMENTrainer)
    tr.params = types.SimpleNamespace(train=types.SimpleNamespace(batch_size=batch_size))
    tr.device, tr.encoder, tr.t_cap = torch.device("cpu"), None, t_cap
    model = types.SimpleNamespace(fused_graph=True, enc_train=None, w1_shadow=object(), fuse_head=True, fuse_project_graph=True,
                                  wgrad_bf16=True, terms=terms, n_classes=6, input_size=D, compute="bf16",
                                  BN_FUSED_MAX_N=COGMENModule.BN_FUSED_MAX_N)
    model.supports_capacity = types.MethodType(COGMENModule.supports_capacity, model)
    tr.model = model
    return tr


def _batch(lengths, T=None, dtype=torch.bfloat16):
    B, T = len(lengths), T or max(lengths)
    N = sum(lengths)
    return dict(input_tensor=torch.zeros(B, T, D, dtype=dtype), speaker_tensor=torch.zeros(B, T, dtype=torch.int64),
                text_length=torch.tensor(lengths, dtype=torch.int64), label=torch.zeros(N, dtype=torch.int64))


def test_bucket_keys_round_n_up_to_256_at_most_b_times_t():
    tr = _trainer()
    assert tr.N_BUCKET == 256
    assert tr.capacity_bucket(_batch([5]))[0] == ("capacity", 4, 70, 256)
    assert tr.capacity_bucket(_batch([64] * 4))[0] == ("capacity", 4, 70, 256)              # N = 256
    assert tr.capacity_bucket(_batch([65, 64, 64, 64]))[0] == ("capacity", 4, 70, 280)      # N = 257 -> 512, clipped to B T
    assert tr.capacity_bucket(_batch([70] * 4))[0] == ("capacity", 4, 70, 280)              # N = 280 = B T
    # a batch larger than train.batch_size or longer than t_cap widens its own bucket
    assert tr.capacity_bucket(_batch([3] * 6, T=80))[0] == ("capacity", 6, 80, 256)


def test_a_batch_of_exactly_the_buckets_shape_still_gets_a_bucket():
    tr = _trainer()
    b = _batch([70] * 4)                                                 # B, T, N == B_cap, T_cap, N_cap
    key, make, fill = tr.capacity_bucket(b)
    assert key == ("capacity", 4, 70, 280)
    static = make()
    assert static["input_tensor"].shape == (4, 70, D) and static["input_tensor"].dtype == torch.bfloat16
    assert static["speaker_tensor"].shape == (4, 70) and static["label"].shape == (280, )
    fill(static, b)
    fill(static, _batch([3, 4]))
    assert static["text_length"].tolist() == [3, 4, 0, 0]


def test_no_bucket_with_the_dead_encoder_above_the_fused_limit_or_off_the_fused_path():
    tr = _trainer(batch_size=32, t_cap=300)
    assert tr.model.BN_FUSED_MAX_N == 8192
    assert tr.capacity_bucket(_batch([256] * 32))[0] == ("capacity", 32, 300, 8192)
    assert tr.capacity_bucket(_batch([256] * 31 + [257])) is None       # N = 8193 -> 8448 rows
    ok = _batch([20] * 8)
    assert tr.capacity_bucket(ok) is not None and tr.all_capacity_buckets(ok)
    tr.encoder = object()                                                # --faithful_dead_encoder
    assert tr.capacity_bucket(ok) is None and tr.all_capacity_buckets(ok) == []
    tr.encoder = None
    assert tr.capacity_bucket(dict(ok, input_tensor=ok["input_tensor"].float())) is None      # bf16 model, fp32 data
    tr.model.fused_graph = False
    assert tr.capacity_bucket(ok) is None and tr.all_capacity_buckets(ok) == []


def test_all_capacity_buckets_has_no_clipped_top_entry():
    tr = _trainer()
    buckets = tr.all_capacity_buckets(_batch([5, 9]))
    assert [k for k, _, _, _ in buckets] == [("capacity", 4, 70, 256)]   # B T = 280: the clipped 280-row bucket is not listed
    tr.t_cap = 130
    assert [k[3] for k, _, _, _ in tr.all_capacity_buckets(_batch([5, 9]))] == [256, 512]       # B T = 520
    big = _trainer(batch_size=32, t_cap=300)
    caps = [k[3] for k, _, _, _ in big.all_capacity_buckets(_batch([5, 9]))]
    assert caps == list(range(256, 8192 + 1, 256))                      # B T = 9600: the list ends at the fused limit


def test_synth_lengths_add_up_to_the_capacity_each_at_most_t_cap():
    for tr in (_trainer(), _trainer(batch_size=4, t_cap=130), _trainer(batch_size=3, t_cap=100)):
        B_cap, T_cap = int(tr.params.train.batch_size), tr.t_cap
        buckets = tr.all_capacity_buckets(_batch([5, 9]))
        assert buckets
        for key, make, fill, synth in buckets:
            static = make()
            synth(static)
            lens = static["text_length"]
            assert lens.shape == (B_cap, ) and int(lens.max()) <= T_cap and int(lens.min()) >= 0
            assert int(lens.sum()) == min(key[3], B_cap * T_cap)


def test_resident_batch_refusals():
    tr = _trainer()
    desc = torch.zeros(8, dtype=torch.int32)
    mk = lambda dt, w=D: types.SimpleNamespace(fused=torch.zeros(10, w, dtype=dt), speaker=torch.zeros(10, dtype=torch.int64),
                                               label=torch.zeros(10, dtype=torch.int64))
    store = mk(torch.bfloat16)
    b = tr.resident_batch(store, desc, 4, 70, 256)
    assert b["desc"] is desc and b["text_length"] is None and b["caps"] == (4, 70, 256)
    assert b["input_tensor"] is store.fused and b["speaker_tensor"] is store.speaker and b["label"] is store.label
    assert tr.resident_eval_batch(store, desc, 4, 70, 128)["caps"] == (4, 70, 128)
    assert tr.resident_batch(mk(torch.float32), desc, 4, 70, 256) is None           # one bf16 term: the store must be bf16
    assert tr.resident_batch(store, desc, 32, 300, 8192 + 128) is None              # above the fused path's node limit
    assert tr.resident_batch(mk(torch.bfloat16, D + 2), desc, 4, 70, 256) is None   # width no multiple of 4
    tr.encoder = object()
    assert tr.resident_batch(store, desc, 4, 70, 256) is None
    tr.encoder = None
    tr.model.fused_graph = False
    assert tr.resident_batch(store, desc, 4, 70, 256) is None
    # the split modes (terms > 1) read the fp32 features
    split = _trainer(terms=3)
    assert split.resident_batch(mk(torch.float32), desc, 4, 70, 256)["caps"] == (4, 70, 256)
    assert split.resident_batch(store, desc, 4, 70, 256) is None


def test_a_bucket_carries_the_models_arguments_alone():
    """forward(**batch) runs on the static dict: no host-side bookkeeping key ("extent") may be in it"""
    tr = _trainer()
    key, make, fill = tr.capacity_bucket(_batch([5, 9]))
    static = make()
    fill(static, _batch([5, 9]))
    fill(static, _batch([3]))
    assert set(static) == {"input_tensor", "speaker_tensor", "text_length", "label"}
