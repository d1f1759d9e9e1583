"""Restatement of one MMGCN training step (oracle.mmgcn.MMGCNOracle's forward, cross entropy, gradients by autograd) in
which every dropout site takes a GIVEN 0/1 keep mask and keep scale instead of drawing one, in float64 (or, as the yardstick
of a fp32 implementation's rounding, in float32), for the tests.

Sites, in the order of the forward (track_mm/mmgcn.py:113-120, track_mm/mmgcn_models.py:382-392), with the layout of their
masks (Mo modalities in the order [a, v, t], N nodes, R3 = Mo N node rows modality-major, FD = 200):
    "lstm"    [T, B, 200]       the BiLSTM's layer-0 output, before layer 1 (nn.LSTM's interlayer dropout; padded rows too)
    "x"       [R3, FD]          the GCNII input, before fcs[0]  (the adjacency is built from the UNDROPPED rows)
    "h0"      [R3, FD]          relu(fcs[0] x), before layer 1  (the residual input h0 itself stays undropped)
    "layers"  [64, R3, FD]      relu(out_l), l = 1..64
    "fe"      [N, Mo 2 FD]      the regrouped cat[x, h] of the node's modalities, before the ReLU in front of smax_fc
A site without a mask is left alone (masks=None: the oracle's eval-mode forward).  The two LSTM layers run as two one-layer
nn.LSTMs on copies of the oracle's parameters; the adjacency is oracle.mmgcn.big_adjacency.
"""
import math

import torch
from torch import nn
from torch.nn import functional as F

from oracle.mmgcn import big_adjacency

FD, NL, LAMDA, ALPHA = 200, 64, 0.5, 0.1
SITES = ("lstm", "x", "h0", "layers", "fe")
_LSTM_NAMES = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")


def _site(t, name, masks, ks, res, dtype):
    """record the site's input (value, and later its gradient through THIS site only), apply the site's mask"""
    t = t.clone()
    t.retain_grad()
    res["pre"][name] = t
    if masks is not None and masks.get(name) is not None:
        t = t * torch.as_tensor(masks[name]).to("cpu", dtype) * ks
    return t


def _one_layer_lstms(lstm, dtype):
    layers = []
    for k in (0, 1):
        one = nn.LSTM(2 * lstm.hidden_size if k else lstm.input_size, lstm.hidden_size, bidirectional=True).to(dtype)
        with torch.no_grad():
            for n in _LSTM_NAMES:
                for suffix in ("", "_reverse"):
                    getattr(one, n + suffix).copy_(getattr(lstm, n.replace("l0", "l%d" % k) + suffix))
        layers.append(one)
    return layers


def mmgcn_step_ref(ref, batch, masks=None, ks=1.0, dtype=torch.float64):
    """``ref``: an oracle.mmgcn.MMGCNOracle (left untouched; its parameters are read in ``dtype``); ``batch``: time-major, one-hot
    speakers.  Returns dict(logits [N, C], loss, grads {oracle parameter name: gradient}, pre {site: the site's input},
    site_grads {site: gradient wrt that input through the site alone}, cat [N, Mo 2 FD] = pre["fe"])."""
    par = {n: p.detach().to("cpu", dtype).clone().requires_grad_() for n, p in ref.named_parameters()}
    feat = lambda k: batch[k].detach().to("cpu", dtype)
    lens = [int(v) for v in batch["text_length"]]
    flatten = lambda f: torch.cat([f[:L, j] for j, L in enumerate(lens)])
    res = {"pre": {}}
    feats, lstms = [], None
    if "a" in ref.modals:
        feats.append(flatten(F.linear(feat("audio_feature"), par["linear_a.weight"], par["linear_a.bias"])))
    if "v" in ref.modals:
        feats.append(flatten(F.linear(feat("visual_feature"), par["linear_v.weight"], par["linear_v.bias"])))
    if "t" in ref.modals:
        lstms = _one_layer_lstms(ref.lstm_l, dtype)
        xl = F.linear(feat("text_feature"), par["linear_l.weight"], par["linear_l.bias"])
        out0, _ = lstms[0](xl)                              # unpacked: over the padded tail too, as the oracle
        out1, _ = lstms[1](_site(out0, "lstm", masks, ks, res, dtype))
        qm = torch.cat([batch["speaker_tensor"][:L, j] for j, L in enumerate(lens)])
        feats.append(flatten(out1) + par["graph_model.speaker_embeddings.weight"][torch.argmax(qm, dim=-1)])
    Mo, N = len(feats), sum(lens)
    adj = big_adjacency(feats, lens)
    gn = "graph_model.graph_net."
    xd = _site(torch.cat(feats), "x", masks, ks, res, dtype)
    h0 = torch.relu(F.linear(xd, par[gn + "fcs.0.weight"], par[gn + "fcs.0.bias"]))
    h = _site(h0, "h0", masks, ks, res, dtype)
    outs = []
    for l in range(1, NL + 1):
        th, W = math.log(LAMDA / l + 1), par[gn + "convs.%d.weight" % (l - 1)]
        hi = adj @ h
        out = th * (torch.cat([hi, h0], 1) @ W) + (1 - th) * ((1 - ALPHA) * hi + ALPHA * h0)
        out.retain_grad()
        outs.append(out)
        h = torch.relu(out)
        if masks is not None and masks.get("layers") is not None:
            h = h * torch.as_tensor(masks["layers"][l - 1]).to("cpu", dtype) * ks
    cat = torch.cat([xd, h], dim=-1)
    cat = torch.cat([cat[N * i:N * (i + 1)] for i in range(Mo)], dim=-1)
    fe = torch.relu(_site(cat, "fe", masks, ks, res, dtype))
    logits = F.linear(fe, par["smax_fc.weight"], par["smax_fc.bias"])
    loss = F.cross_entropy(logits, batch["label"])
    loss.backward()
    grads = {n: p.grad for n, p in par.items() if p.grad is not None and not n.startswith("lstm_l.")}
    if lstms is not None:
        for k, one in enumerate(lstms):
            for n in _LSTM_NAMES:
                for suffix in ("", "_reverse"):
                    grads["lstm_l." + n.replace("l0", "l%d" % k) + suffix] = getattr(one, n + suffix).grad
    res["site_grads"] = {k: v.grad for k, v in res["pre"].items()}
    res["site_grads"]["layers"] = torch.stack([o.grad for o in outs])
    res["pre"] = {k: v.detach() for k, v in res["pre"].items()}
    res["pre"]["layers"] = torch.stack(outs).detach()
    res.update(logits=logits.detach(), loss=loss.detach(), grads=grads, cat=res["pre"]["fe"])
    return res
