"""Host logic of the config-4 rollout MLP (no GPU): FusedMLP's one-kernel
form (the tensors sn_puct_mlp_seats / sn_puct_rollouts read) -- layer 1 per
seat through the [W1 | b1 | 0] rows of w1s with the ones feature, the card
column w1c added per candidate, layer 2 through [W2 | b2 | 0] with the ones
pass-through row, the head [wh | bh | 0] -- restates the module's own
forward on the full [card, obs] rows; other layouts get no fused form; and
refresh_from copies new weights into the same tensors (the captured
hipGraphs stay valid)."""
import torch

from rl_6_nimmt.puct import FusedMLP, make_actor
from rl_6_nimmt.utils.nets import MultiHeadedMLP


def _fused_forward(fz, obs, cards, n_cur):
    """the kernels' arithmetic in f32, without their bf16 roundings of the
    activations: what the padded tensors encode"""
    w1c, w2p, head, w1s = (t.float() for t in fz)
    S = obs.shape[0]
    seat = torch.zeros((S, 64))
    seat[:, 1:48] = obs
    seat[:, 48] = 1.0  # the ones feature
    base = seat @ w1s.t()  # [S, 128]: rows >= H are 0 except the ones row H
    h1 = torch.relu(base[:, :112].repeat_interleave(n_cur, dim=0) + cards[:, None] * w1c[None, :])
    h2 = torch.relu(h1 @ w2p.t())  # [R, 128]: the ones pass-through row H2 carries the head bias
    return h2 @ head


def test_fused_form_restates_module_forward():
    torch.manual_seed(0)
    net = make_actor().to(torch.bfloat16)
    fm = FusedMLP.of(net)
    fz = fm.fused()
    assert fz is not None
    w1c, w2p, head, w1s = fz
    assert w1c.shape == (112,) and w2p.shape == (128, 112) and head.shape == (128,) and w1s.shape == (128, 64)
    assert float(w1s[100, 48]) == 1.0 and float(w2p[100, 100]) == 1.0  # ones feature / pass-through
    S, n_cur = 37, 5
    obs = (torch.rand(S, 47) * 2 - 1).to(torch.bfloat16).float()
    cards = (torch.rand(S * n_cur) * 2 - 1).to(torch.bfloat16).float()
    rows = torch.cat((cards[:, None], obs.repeat_interleave(n_cur, dim=0)), dim=1)  # [R, 48]
    with torch.no_grad():
        (want,) = net.float()(rows)
    got = _fused_forward(fz, obs, cards, n_cur)
    assert torch.allclose(got, want[:, 0], rtol=1e-5, atol=1e-5)


def test_fused_form_rejects_other_layouts():
    torch.manual_seed(0)
    relu = torch.nn.ReLU()
    for net in (MultiHeadedMLP(47, hidden_sizes=(32, 32), head_sizes=(1,), activation=relu,
                               head_activations=(None,)).to(torch.bfloat16),   # another input width
                MultiHeadedMLP(48, hidden_sizes=(40, 24, 16), head_sizes=(1,), activation=relu,
                               head_activations=(None,)).to(torch.bfloat16),   # three hidden layers
                make_actor()):                                                 # fp32
        assert FusedMLP.of(net).fused() is None  # these run sn_puct_rows + the module's forward


def test_refresh_from_updates_in_place():
    torch.manual_seed(1)
    actor = make_actor().to(torch.bfloat16)
    net = FusedMLP.of(make_actor().to(torch.bfloat16))
    net.refresh_from(actor)
    fz = net.fused()
    before = [t.data_ptr() for t in fz] + [net.head_w.data_ptr(), net.head_b.data_ptr()]
    with torch.no_grad():
        for p in actor.parameters():
            p.add_(0.25)
    assert net.refresh_from(actor)
    after = [t.data_ptr() for t in net.fused()] + [net.head_w.data_ptr(), net.head_b.data_ptr()]
    assert before == after
    fresh = FusedMLP.of(actor)
    for a, b in zip(net.fused(), fresh.fused()):
        assert torch.equal(a, b)
    assert torch.equal(net.head_w, fresh.head_w) and torch.equal(net.head_b, fresh.head_b)
    other = MultiHeadedMLP(48, hidden_sizes=(64,), head_sizes=(1,), activation=torch.nn.ReLU(), head_activations=(None,))
    assert not net.refresh_from(other)


def test_crafted_actor_logits_are_card_only_and_far_apart():
    """the design condition of tests/test_gpu_puct_players.py, with no GPU involved: the crafted weights give
    logit = +-S * nrm(card) for every one of the 104 cards whatever the observation holds -- through FusedMLP's
    factored restatement (the tensors the MFMA kernels read), the module in bf16 (the root policy's path) and
    the module in f32 -- and two distinct cards' logits lie >= 150 apart, in card order.  Past 104 every other
    candidate's exp(x - max) is exactly 0 in float32 (exp underflows below -103.98; the margin covers the
    device's approximate __expf), so Categorical.sample returns the preferred card for every uniform."""
    from test_gpu_puct_players import S_LOGIT, crafted_weights

    torch.manual_seed(0)
    K = 5  # observations per card
    x = -1.0 + 2.0 * torch.arange(104, dtype=torch.float32) / 103.0  # nrm(card, 0, 103)
    obs = (torch.rand(104 * K, 47) * 2.04 - 1.02).to(torch.bfloat16).float()
    for polarity in (1, -1):
        net = make_actor()
        net.load_state_dict(crafted_weights(polarity))
        card32 = x.repeat_interleave(K)
        card16 = card32.to(torch.bfloat16).float()  # the rounding of the bf16 rows
        with torch.no_grad():
            (f32,) = net(torch.cat((card32[:, None], obs), dim=1))
            net16 = make_actor()
            net16.load_state_dict(crafted_weights(polarity))
            net16 = net16.to(torch.bfloat16)
            (b16,) = net16(torch.cat((card16[:, None], obs), dim=1).to(torch.bfloat16))
            fz = FusedMLP.of(net16).fused()
            assert fz is not None
            fused = _fused_forward(fz, obs, card16, 1)
        for name, got, card in (("f32", f32[:, 0], card32), ("bf16", b16[:, 0].float(), card16), ("fused", fused, card16)):
            got = got.reshape(104, K)
            assert torch.equal(got, got[:, :1].expand(-1, K)), name  # no observation column reaches the logit
            assert torch.equal(got[:, 0], polarity * S_LOGIT * card.reshape(104, K)[:, 0]), name  # +-S nrm(card), exactly
            gaps = polarity * (got[1:, 0] - got[:-1, 0])
            assert float(gaps.min()) >= 150.0, (name, polarity, float(gaps.min()))


def test_root_choice_restatement_reproduces_reference_formula():
    """the numpy float64 restatement of PUCTAgent._compute_pucts + argmax that test_gpu_puct_players.py's host
    model chooses root moves with, on the statistics words the kernels keep: every recorded case of the
    reference's own numbers (golden F5: PUCT values bit for bit, NaN where the reference has NaN, and the
    choice)"""
    import json
    import os

    import numpy as np

    from conftest import GOLDEN
    from test_gpu_puct_players import puct_choose_ref

    with open(os.path.join(GOLDEN, "puct_math.json")) as f:
        d = json.load(f)
    filled = 0
    for i, c in enumerate(d["cases"]):
        n = len(c["legal"])
        st, hist = np.zeros(24, dtype=np.int32), np.zeros(172, dtype=np.int32)
        allo = []
        for k, outs in enumerate(c["outcomes"]):
            st[k], st[10 + k] = int(sum(outs)), len(outs)
            allo += outs
        st[20] = len(allo)
        if allo:
            st[21], st[22] = int(min(allo)), int(max(allo))
        for o in allo:
            hist[int(o) + 171] += 1
        filled += len(allo) >= 10 and any(not outs for outs in c["outcomes"])
        choice, pucts = puct_choose_ref(st, hist, np.array(c["probs"], dtype=np.float32), n, d["c_puct"])
        want = np.array([np.nan if v is None else v for v in c["pucts"]])
        assert np.array_equal(pucts, want, equal_nan=True), i
        assert choice == c["choice"], i
    assert filled > 0  # the median fill of unvisited moves is among the cases
