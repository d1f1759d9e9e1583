"""CPU: the launch sequence of the hidden-100 encoders (erc_amd/rnn.py) -- which C entry point, in which order, with which
arguments -- for one forward + backward of ``BiLSTM2`` (packed padded rows; compact rows with ``zero_to``; ``t_dev``) and of
``BiGRU2`` (padded rows; ``t_dev``).  The C-ABI calls are recorded with ``capi.start_recording()`` under a fake ``lib()`` that
executes nothing; the hoisted products (``engine.linear_fwd`` / ``linear_wgrad``) are recorded in the same list under their own
names.  Operands are named stand-ins, so a list reads as the step does.  The expected lists are written out below: they are
what the two separate classes this module once held issued on the same operands, and ``BiRNN2`` must issue the same."""
import pytest

H = 100


class Named:
    """stand-in for a tensor: passes through capi._call untouched (it is no torch.Tensor), slices keep their origin"""

    def __init__(self, name):
        self.name, self.device = name, "cpu"

    def __getitem__(self, idx):
        return Named("%s[:, %d:]" % (self.name, idx[1].start))

    def __repr__(self):
        return self.name


class _Flat:
    def __init__(self, G):
        names = [b % k + r for k in (0, 1) for b in ("weight_ih_l%d", "bias_ih_l%d", "weight_hh_l%d", "bias_hh_l%d")
                 for r in ("", "_reverse")]
        self.offsets = {"rnn." + n: 1000 * i for i, n in enumerate(names)}

    def w(self, name):
        return Named(name[4:])


def _workspace(keys, prefix, rows_key, rows):
    two = lambda n: [Named(n + "0"), Named(n + "1")]
    ws = {k: two(k) for k in keys}
    ws.update(H0=Named("H0"), H0d=Named("H0d"), dH0d=Named("dH0d"))
    return {prefix + "rnn.": ws, rows_key: rows}


def _plain(v):
    if isinstance(v, Named):
        return v.name
    return tuple(_plain(x) for x in v) if isinstance(v, tuple) else v


@pytest.fixture
def record(monkeypatch):
    from erc_amd import capi, rnn

    class _Lib:
        def __getattr__(self, name):
            def call(*a):
                capi._record.append((name, a))
                return 0
            return call
    monkeypatch.setattr(capi, "_lib", _Lib())
    monkeypatch.setattr(capi, "stream", lambda: "stream")
    for fn in ("linear_fwd", "linear_wgrad"):
        monkeypatch.setattr(rnn, fn, lambda pl, *a, _fn=fn, **kw: capi._record.append(
            (_fn, a + tuple(sorted(kw.items())))))

    def run(cell, fwd, bwd, rows):
        if cell == "lstm":
            enc = rnn.BiLSTM2(_Flat(4), "rnn.", 20)
            store = _workspace(("GX", "gates", "Cst", "Hprev", "dGX"), "lstm:", "lstm_rows", rows)
        else:
            enc = rnn.BiGRU2(_Flat(3), "rnn.", 20)
            store = _workspace(("GX", "gates", "ghn", "Hprev", "dGX", "dGH"), "gru:", "gru_rows", rows)
        assert enc.drop_p == (0.4 if cell == "lstm" else 0.5)
        capi.start_recording()
        try:
            enc.forward("pl", Named("x"), 20, rows, *fwd[0], Named("out"), fwd[1], store=store, **fwd[2])
            enc.backward("pl", Named("dout"), *bwd[0], **bwd[1])
        finally:
            rec = capi.stop_recording()
        return [(n, _plain(a)) for n, a in rec]
    return run


def cases():
    """name -> (cell, forward arguments (B, T, sb, st, lengths, training, rng | ldo | keywords), backward (lddo | keywords), rows)"""
    lens, rng, td = Named("lengths"), Named("rng"), Named("t_dev")
    return {
        "lstm_packed": ("lstm", ((2, 9, 9, 1, lens, True, rng), 200, {}), ((200, ), {}), 18),
        "lstm_compact_zero_to": ("lstm", ((2, 9, 9, 1, lens, True, rng), 300, dict(node_off=Named("node_off"), node_row=Named("node_row"))),
                                 ((300, ), dict(zero_to=16)), 14),
        "lstm_t_dev": ("lstm", ((3, 9, 1, 3, None, False, rng), 200, dict(t_dev=td)), ((200, ), dict(dx=Named("dx"), lddx=20)), 27),
        "gru_padded": ("gru", ((3, 9, 1, 3, None, True, rng), 200, {}), ((200, ), dict(dx=Named("dx"), lddx=20)), 27),
        "gru_t_dev": ("gru", ((3, 9, 1, 3, None, True, rng), 200, dict(t_dev=td)), ((200, ), {}), 27),
    }


# recorded from BiLSTM2 / BiGRU2 as two separate classes (454352 = 0x6EED0 and 388816 = 0x5EED0: the layer-0 dropout streams)
EXPECTED = {'gru_padded': [('linear_fwd', ('x', 20, None, 'weight_ih_l0', 'bias_ih_l0', 'GX0', 600, 27, 600, 20, ('x_bf16', False))),
                ('erc_gru100_scan_fwd',
                 ('GX0', 600, 'weight_hh_l0', 'bias_hh_l0', None, None, 1, 3, 3, 9, 'H0', 200, 'H0d', 200, 0.5, 'rng', 454352, 'gates0', 'ghn0',
                  'Hprev0', 'stream')),
                ('linear_fwd', ('H0d', 200, None, 'weight_ih_l1', 'bias_ih_l1', 'GX1', 600, 27, 600, 200)),
                ('erc_gru100_scan_fwd',
                 ('GX1', 600, 'weight_hh_l1', 'bias_hh_l1', None, None, 1, 3, 3, 9, 'out', 200, None, 0, 0.0, None, 0, 'gates1', 'ghn1', 'Hprev1',
                  'stream')),
                ('erc_gru100_scan_bwd',
                 ('weight_hh_l1', None, None, 1, 3, 3, 9, 'gates1', 'ghn1', 'Hprev1', 'dout', 200, 0.0, None, 0, 'dGX1', 'dGH1', 'stream')),
                ('linear_wgrad', ('dGX1', 600, 'H0d', 200, None, 600, 200, 27, 8000, 10000, ('defer', True), ('x_bf16', False))),
                ('linear_wgrad', ('dGH1[:, 0:]', 600, 'Hprev1[:, 0:]', 200, None, 300, 100, 27, 12000, 14000, ('defer', True))),
                ('linear_wgrad', ('dGH1[:, 300:]', 600, 'Hprev1[:, 100:]', 200, None, 300, 100, 27, 42000, 14300, ('defer', True))),
                ('erc_gemm_f32',
                 ('dGX1', 600, 0, None, 'weight_ih_l1', 200, 1, None, 'dH0d', 200, 27, 200, 600, 1, 0, 0, None, 0, None, 0, None, 0, 1.0, 0.0, None,
                  0, 'stream')),
                ('erc_gru100_scan_bwd',
                 ('weight_hh_l0', None, None, 1, 3, 3, 9, 'gates0', 'ghn0', 'Hprev0', 'dH0d', 200, 0.5, 'rng', 454352, 'dGX0', 'dGH0', 'stream')),
                ('linear_wgrad', ('dGX0', 600, 'x', 20, None, 600, 20, 27, 0, 2000, ('defer', True), ('x_bf16', False))),
                ('linear_wgrad', ('dGH0[:, 0:]', 600, 'Hprev0[:, 0:]', 200, None, 300, 100, 27, 4000, 6000, ('defer', True))),
                ('linear_wgrad', ('dGH0[:, 300:]', 600, 'Hprev0[:, 100:]', 200, None, 300, 100, 27, 34000, 6300, ('defer', True))),
                ('erc_gemm_f32',
                 ('dGX0', 600, 0, None, 'weight_ih_l0', 20, 1, None, 'dx', 20, 27, 20, 600, 1, 0, 0, None, 0, None, 0, None, 0, 1.0, 0.0, None, 0,
                  'stream'))],
 'gru_t_dev': [('linear_fwd', ('x', 20, None, 'weight_ih_l0', 'bias_ih_l0', 'GX0', 600, 27, 600, 20, ('x_bf16', False))),
               ('erc_gru100_scan_fwd_tcap',
                ('GX0', 600, 'weight_hh_l0', 'bias_hh_l0', 1, 3, 3, 9, 't_dev', 'H0', 200, 'H0d', 200, 0.5, 'rng', 454352, 'gates0', 'ghn0', 'Hprev0',
                 'stream')),
               ('linear_fwd', ('H0d', 200, None, 'weight_ih_l1', 'bias_ih_l1', 'GX1', 600, 27, 600, 200)),
               ('erc_gru100_scan_fwd_tcap',
                ('GX1', 600, 'weight_hh_l1', 'bias_hh_l1', 1, 3, 3, 9, 't_dev', 'out', 200, None, 0, 0.0, None, 0, 'gates1', 'ghn1', 'Hprev1',
                 'stream')),
               ('erc_gru100_scan_bwd_tcap',
                ('weight_hh_l1', 1, 3, 3, 9, 't_dev', 'gates1', 'ghn1', 'Hprev1', 'dout', 200, 0.0, None, 0, 'dGX1', 'dGH1', 'stream')),
               ('linear_wgrad', ('dGX1', 600, 'H0d', 200, None, 600, 200, 27, 8000, 10000, ('defer', True), ('x_bf16', False))),
               ('linear_wgrad', ('dGH1[:, 0:]', 600, 'Hprev1[:, 0:]', 200, None, 300, 100, 27, 12000, 14000, ('defer', True))),
               ('linear_wgrad', ('dGH1[:, 300:]', 600, 'Hprev1[:, 100:]', 200, None, 300, 100, 27, 42000, 14300, ('defer', True))),
               ('erc_gemm_f32',
                ('dGX1', 600, 0, None, 'weight_ih_l1', 200, 1, None, 'dH0d', 200, 27, 200, 600, 1, 0, 0, None, 0, None, 0, None, 0, 1.0, 0.0, None, 0,
                 'stream')),
               ('erc_gru100_scan_bwd_tcap',
                ('weight_hh_l0', 1, 3, 3, 9, 't_dev', 'gates0', 'ghn0', 'Hprev0', 'dH0d', 200, 0.5, 'rng', 454352, 'dGX0', 'dGH0', 'stream')),
               ('linear_wgrad', ('dGX0', 600, 'x', 20, None, 600, 20, 27, 0, 2000, ('defer', True), ('x_bf16', False))),
               ('linear_wgrad', ('dGH0[:, 0:]', 600, 'Hprev0[:, 0:]', 200, None, 300, 100, 27, 4000, 6000, ('defer', True))),
               ('linear_wgrad', ('dGH0[:, 300:]', 600, 'Hprev0[:, 100:]', 200, None, 300, 100, 27, 34000, 6300, ('defer', True)))],
 'lstm_compact_zero_to': [('linear_fwd', ('x', 20, 'node_row', 'weight_ih_l0', 'bias_ih_l0', 'GX0', 800, 14, 800, 20, ('x_bf16', False))),
                          ('erc_lstm_scan_fwd',
                           ('GX0', 800, 'weight_hh_l0', 'bias_hh_l0', 'lengths', 'node_off', 9, 1, 2, 9, 'H0', 200, 'H0d', 200, 0.4, 'rng', 388816,
                            'gates0', 'Cst0', 'Hprev0', 'stream')),
                          ('linear_fwd', ('H0d', 200, None, 'weight_ih_l1', 'bias_ih_l1', 'GX1', 800, 14, 800, 200)),
                          ('erc_lstm_scan_fwd',
                           ('GX1', 800, 'weight_hh_l1', 'bias_hh_l1', 'lengths', 'node_off', 9, 1, 2, 9, 'out', 300, None, 0, 0.0, None, 0, 'gates1',
                            'Cst1', 'Hprev1', 'stream')),
                          ('erc_lstm_scan_bwd_cap',
                           ('weight_hh_l1', 'lengths', 'node_off', 9, 1, 2, 9, 'gates1', 'Cst1', 'dout', 300, 0.0, None, 0, 'dGX1', 16, 'stream')),
                          ('linear_wgrad', ('dGX1', 800, 'H0d', 200, None, 800, 200, 14, 8000, 10000, ('defer', True), ('x_bf16', False))),
                          ('linear_wgrad', ('dGX1[:, 0:]', 800, 'Hprev1[:, 0:]', 200, None, 400, 100, 14, 12000, 14000, ('defer', True))),
                          ('linear_wgrad', ('dGX1[:, 400:]', 800, 'Hprev1[:, 100:]', 200, None, 400, 100, 14, 52000, 14400, ('defer', True))),
                          ('erc_gemm_f32',
                           ('dGX1', 800, 0, None, 'weight_ih_l1', 200, 1, None, 'dH0d', 200, 14, 200, 800, 1, 0, 0, None, 0, None, 0, None, 0, 1.0,
                            0.0, None, 0, 'stream')),
                          ('erc_lstm_scan_bwd_cap',
                           ('weight_hh_l0', 'lengths', 'node_off', 9, 1, 2, 9, 'gates0', 'Cst0', 'dH0d', 200, 0.4, 'rng', 388816, 'dGX0', 16,
                            'stream')),
                          ('linear_wgrad', ('dGX0', 800, 'x', 20, 'node_row', 800, 20, 14, 0, 2000, ('defer', True), ('x_bf16', False))),
                          ('linear_wgrad', ('dGX0[:, 0:]', 800, 'Hprev0[:, 0:]', 200, None, 400, 100, 14, 4000, 6000, ('defer', True))),
                          ('linear_wgrad', ('dGX0[:, 400:]', 800, 'Hprev0[:, 100:]', 200, None, 400, 100, 14, 44000, 6400, ('defer', True)))],
 'lstm_packed': [('linear_fwd', ('x', 20, None, 'weight_ih_l0', 'bias_ih_l0', 'GX0', 800, 18, 800, 20, ('x_bf16', False))),
                 ('erc_lstm_scan_fwd',
                  ('GX0', 800, 'weight_hh_l0', 'bias_hh_l0', 'lengths', None, 9, 1, 2, 9, 'H0', 200, 'H0d', 200, 0.4, 'rng', 388816, 'gates0', 'Cst0',
                   'Hprev0', 'stream')),
                 ('linear_fwd', ('H0d', 200, None, 'weight_ih_l1', 'bias_ih_l1', 'GX1', 800, 18, 800, 200)),
                 ('erc_lstm_scan_fwd',
                  ('GX1', 800, 'weight_hh_l1', 'bias_hh_l1', 'lengths', None, 9, 1, 2, 9, 'out', 200, None, 0, 0.0, None, 0, 'gates1', 'Cst1',
                   'Hprev1', 'stream')),
                 ('erc_lstm_scan_bwd', ('weight_hh_l1', 'lengths', None, 9, 1, 2, 9, 'gates1', 'Cst1', 'dout', 200, 0.0, None, 0, 'dGX1', 'stream')),
                 ('linear_wgrad', ('dGX1', 800, 'H0d', 200, None, 800, 200, 18, 8000, 10000, ('defer', True), ('x_bf16', False))),
                 ('linear_wgrad', ('dGX1[:, 0:]', 800, 'Hprev1[:, 0:]', 200, None, 400, 100, 18, 12000, 14000, ('defer', True))),
                 ('linear_wgrad', ('dGX1[:, 400:]', 800, 'Hprev1[:, 100:]', 200, None, 400, 100, 18, 52000, 14400, ('defer', True))),
                 ('erc_gemm_f32',
                  ('dGX1', 800, 0, None, 'weight_ih_l1', 200, 1, None, 'dH0d', 200, 18, 200, 800, 1, 0, 0, None, 0, None, 0, None, 0, 1.0, 0.0, None,
                   0, 'stream')),
                 ('erc_lstm_scan_bwd',
                  ('weight_hh_l0', 'lengths', None, 9, 1, 2, 9, 'gates0', 'Cst0', 'dH0d', 200, 0.4, 'rng', 388816, 'dGX0', 'stream')),
                 ('linear_wgrad', ('dGX0', 800, 'x', 20, None, 800, 20, 18, 0, 2000, ('defer', True), ('x_bf16', False))),
                 ('linear_wgrad', ('dGX0[:, 0:]', 800, 'Hprev0[:, 0:]', 200, None, 400, 100, 18, 4000, 6000, ('defer', True))),
                 ('linear_wgrad', ('dGX0[:, 400:]', 800, 'Hprev0[:, 100:]', 200, None, 400, 100, 18, 44000, 6400, ('defer', True)))],
 'lstm_t_dev': [('linear_fwd', ('x', 20, None, 'weight_ih_l0', 'bias_ih_l0', 'GX0', 800, 27, 800, 20, ('x_bf16', False))),
                ('erc_lstm_scan_fwd_tcap',
                 ('GX0', 800, 'weight_hh_l0', 'bias_hh_l0', 1, 3, 3, 9, 't_dev', 'H0', 200, 'H0d', 200, 0.0, 'rng', 388816, 'gates0', 'Cst0',
                  'Hprev0', 'stream')),
                ('linear_fwd', ('H0d', 200, None, 'weight_ih_l1', 'bias_ih_l1', 'GX1', 800, 27, 800, 200)),
                ('erc_lstm_scan_fwd_tcap',
                 ('GX1', 800, 'weight_hh_l1', 'bias_hh_l1', 1, 3, 3, 9, 't_dev', 'out', 200, None, 0, 0.0, None, 0, 'gates1', 'Cst1', 'Hprev1',
                  'stream')),
                ('erc_lstm_scan_bwd_tcap', ('weight_hh_l1', 1, 3, 3, 9, 't_dev', 'gates1', 'Cst1', 'dout', 200, 0.0, None, 0, 'dGX1', 'stream')),
                ('linear_wgrad', ('dGX1', 800, 'H0d', 200, None, 800, 200, 27, 8000, 10000, ('defer', True), ('x_bf16', False))),
                ('linear_wgrad', ('dGX1[:, 0:]', 800, 'Hprev1[:, 0:]', 200, None, 400, 100, 27, 12000, 14000, ('defer', True))),
                ('linear_wgrad', ('dGX1[:, 400:]', 800, 'Hprev1[:, 100:]', 200, None, 400, 100, 27, 52000, 14400, ('defer', True))),
                ('erc_gemm_f32',
                 ('dGX1', 800, 0, None, 'weight_ih_l1', 200, 1, None, 'dH0d', 200, 27, 200, 800, 1, 0, 0, None, 0, None, 0, None, 0, 1.0, 0.0, None,
                  0, 'stream')),
                ('erc_lstm_scan_bwd_tcap',
                 ('weight_hh_l0', 1, 3, 3, 9, 't_dev', 'gates0', 'Cst0', 'dH0d', 200, 0.0, 'rng', 388816, 'dGX0', 'stream')),
                ('linear_wgrad', ('dGX0', 800, 'x', 20, None, 800, 20, 27, 0, 2000, ('defer', True), ('x_bf16', False))),
                ('linear_wgrad', ('dGX0[:, 0:]', 800, 'Hprev0[:, 0:]', 200, None, 400, 100, 27, 4000, 6000, ('defer', True))),
                ('linear_wgrad', ('dGX0[:, 400:]', 800, 'Hprev0[:, 100:]', 200, None, 400, 100, 27, 44000, 6400, ('defer', True))),
                ('erc_gemm_f32',
                 ('dGX0', 800, 0, None, 'weight_ih_l0', 20, 1, None, 'dx', 20, 27, 20, 800, 1, 0, 0, None, 0, None, 0, None, 0, 1.0, 0.0, None, 0,
                  'stream'))]}


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_launch_sequence_is_the_recorded_one(record, name):
    got = record(*cases()[name])
    want = EXPECTED[name]
    assert [n for n, _ in got] == [n for n, _ in want]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, g, w)


def test_t_dev_is_refused_with_lengths_or_compact_rows_and_the_gru_has_no_zero_to(record):
    from erc_amd import capi
    with pytest.raises(capi.ErcGraftError, match="t_dev is the unpacked padded-row form"):
        record("lstm", ((2, 9, 1, 2, Named("lengths"), False, None), 200, dict(t_dev=Named("t_dev"))), ((200, ), {}), 18)
    with pytest.raises(capi.ErcGraftError, match="zero_to"):
        record("gru", ((2, 9, 1, 2, None, False, None), 200, {}), ((200, ), dict(zero_to=20)), 18)
