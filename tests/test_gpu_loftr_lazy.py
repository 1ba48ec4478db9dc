"""The lazy ``conf_matrix`` form of the LoFTR matcher on the MI355X (``hip_conf_matrix = "lazy"`` / ``forward(data, conf_matrix="lazy")``:
``ophip_coarse_match_2d[_masked]`` with ``conf == NULL``) against the eager form of the same call: every match list bit for bit, on plain,
masked and scaled calls, at V > 1, with a shared and with per-pair queries, at equal and at different grid sizes; the ``conf_matrix``
object; the memory the form saves; the eager re-run after an exact row tie.  Shapes: views of 64 x 80 (coarse 8 x 10, L0 = 80) against a
query of 96 x 128 (coarse 12 x 16, L1 = 192) -- a ragged tile edge, two different grids and a batch."""
import copy

import pytest
import torch

from onepose_st_amd import hip, loftr
from onepose_st_amd.lazy_conf import LazyConfMatrixBase
from onepose_st_amd.synthetic import make_synthetic_loftr_state_dict
from tests.loftr_helpers import planted_grids

pytestmark = pytest.mark.gpu

VIEW, QUERY = (64, 80), (96, 128)
LISTS_EQUAL = ("b_ids", "i_ids", "j_ids", "m_bids", "gt_mask")
LISTS_BITS = ("mconf", "mkpts0_c", "mkpts1_c", "expec_f", "mkpts0_f", "mkpts1_f")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    hip.load()
    return torch.device("cuda:0")


def _matcher(dev, sd, **top):
    cfg = copy.deepcopy(loftr.default_cfg)
    for k, v in top.items():
        if isinstance(v, dict):
            cfg[k].update(v)
        else:
            cfg[k] = v
    m = loftr.LoFTR_for_OnePose_Plus(cfg).eval()
    m.load_state_dict(sd, strict=True)
    return m.to(dev)


@pytest.fixture(scope="module")
def sd():
    return make_synthetic_loftr_state_dict(0)


@pytest.fixture(scope="module")
def matcher(dev, sd):
    return _matcher(dev, sd)


def _planted_hook(dev, V, hw0, hw1, shared, seed=3):
    """planted backbone-output features for V pairs (``tests.loftr_helpers.planted_grids``); ``shared``: one query for all pairs -- every
    view then carries pair 0's content under its own noise, so that every pair has matches"""
    g0c, g1c = (hw0[0] // 8, hw0[1] // 8), (hw1[0] // 8, hw1[1] // 8)
    x0, g0, x1, g1 = planted_grids(g0c, g1c, batch=V, seed=seed)
    if shared:
        g = torch.Generator().manual_seed(seed + 100)
        x0 = x0[:1] + 0.05 * torch.randn(x0.shape, generator=g)
        g0 = g0[:1] + 0.05 * torch.randn(g0.shape, generator=g)
        x1, g1 = x1[:1], g1[:1]
    cl = lambda t: t.permute(0, 2, 3, 1).reshape(t.shape[0], -1, 128).contiguous().to(dev)
    feats = (x0.to(dev), cl(g0), x1.to(dev), cl(g1))
    return lambda fc0, ff0, fc1, ff1: feats


def _inputs(dev, V, hw0, hw1, shared, extra):
    V1 = 1 if shared else V
    data = {"image0": torch.zeros(V, 1, *hw0, device=dev), "image1": torch.zeros(V1, 1, *hw1, device=dev)}
    if extra == "masks":                                            # a padded right and bottom band on each image
        m0 = torch.ones(V, hw0[0] // 8, hw0[1] // 8, dtype=torch.bool, device=dev)
        m1 = torch.ones(V1, hw1[0] // 8, hw1[1] // 8, dtype=torch.bool, device=dev)
        m0[:, -1:, :], m0[:, :, -1:] = False, False
        m1[:, -1:, :], m1[:, :, -2:] = False, False
        if V > 1:                                                   # another extent for the last pair: the border is per pair
            m0[-1, -2:, :] = False
        data.update({"mask0": m0, "mask1": m1})
    if extra == "scales":
        data["scale0"] = torch.tensor([[1.25, 0.75 + 0.5 * k] for k in range(V)], device=dev)
        data["scale1"] = torch.tensor([[2.0 - 0.25 * k, 1.5] for k in range(V1)], device=dev)
    return data


def _run(m, data, hook, **kw):
    m.feature_hook = hook
    try:
        d = dict(data)
        m(d, **kw)
    finally:
        m.feature_hook = None
    return d


def _same_lists(lazy, eager, what=""):
    K = eager["b_ids"].shape[0]
    assert K > 0, what                                              # the comparison cannot pass on empty lists
    for k in LISTS_EQUAL:
        assert lazy[k].dtype == eager[k].dtype and lazy[k].tolist() == eager[k].tolist(), (k, what)
    for k in LISTS_BITS:
        assert lazy[k].dtype == eager[k].dtype and torch.equal(lazy[k], eager[k]), (k, what)
    return K


@pytest.mark.parametrize("extra", ["plain", "masks", "scales"])
@pytest.mark.parametrize("hw1", [VIEW, QUERY], ids=["equal_grids", "two_grids"])
@pytest.mark.parametrize("shared", [True, False], ids=["shared_query", "pair_queries"])
@pytest.mark.parametrize("V", [1, 3])
def test_lazy_lists_equal_the_eager_forms(matcher, dev, V, shared, hw1, extra):
    hook = _planted_hook(dev, V, VIEW, hw1, shared)
    data = _inputs(dev, V, VIEW, hw1, shared, extra)
    eager = _run(matcher, data, hook)
    before = matcher.lazy_reruns
    lazy = _run(matcher, data, hook, conf_matrix="lazy")
    K = _same_lists(lazy, eager, (V, shared, hw1, extra))
    assert matcher.lazy_reruns == before                            # no tie in random features: the lists are the lazy kernels' own
    if extra != "masks":                                            # (the padded bands leave few cells inside the border)
        assert sorted(set(eager["b_ids"].tolist())) == list(range(V)), "every pair has matches"
    print(f"V={V} shared={shared} hw1={hw1} {extra}: K={K}")
    assert isinstance(eager["conf_matrix"], torch.Tensor) and not isinstance(lazy["conf_matrix"], torch.Tensor)
    _same_lists(_run(matcher, data, hook, conf_matrix="eager"), eager)


def test_config_key_and_conf_matrix_object(matcher, dev, sd):
    V, L0, L1 = 3, 80, 192
    lazy_m = _matcher(dev, sd, hip_conf_matrix="lazy")
    hook = _planted_hook(dev, V, VIEW, QUERY, shared=True)
    for extra in ("plain", "masks"):
        data = _inputs(dev, V, VIEW, QUERY, True, extra)
        eager = _run(matcher, data, hook)
        lazy = _run(lazy_m, data, hook)                             # the config key, no keyword
        _same_lists(lazy, eager, extra)
        cm = lazy["conf_matrix"]
        assert isinstance(cm, loftr.LazyConfMatrix) and isinstance(cm, LazyConfMatrixBase) and not isinstance(cm, torch.Tensor)
        assert cm._t is None and tuple(cm.shape) == (V, L0, L1) and cm.dtype == torch.float32 and cm.device == eager["conf_matrix"].device
        assert cm.size(2) == L1 and cm.dim() == 3 and len(cm) == V and cm._t is None           # answered without materialising
        held = sum(t.numel() for t in (cm._x0, cm._x1))
        assert held == V * (L0 + L1) * 256                          # the final rows and nothing V x L0 x L1
        if extra == "plain":
            got = torch.max(cm, dim=2)[0]                           # a torch function materialises first
            assert cm._t is not None and torch.equal(got, eager["conf_matrix"].max(dim=2)[0])
        else:
            assert torch.equal(cm[1, :7], eager["conf_matrix"][1, :7]) and cm._t is not None      # so does indexing
        assert torch.equal(cm.materialize(), eager["conf_matrix"]) and cm._x0 is None and cm._x1 is None
        assert torch.equal(torch.as_tensor(cm.materialize()), eager["conf_matrix"])
        _same_lists(_run(lazy_m, data, hook, conf_matrix="eager"), eager)                          # the keyword overrides the key
        assert isinstance(_run(lazy_m, data, hook, conf_matrix="eager")["conf_matrix"], torch.Tensor)


def test_real_backbone_fine_off_and_fine_only(dev, sd):
    """through the real backbone at the same sizes.  Random weights on random images give (almost) no match above thr = 0.2, so this
    matcher runs with thr = 1e-6 (practically every mutual nearest neighbour inside the border is a match) on a query that holds view 0 at an
    8-aligned offset; ``enable_fine_matching=False`` and the fine-only branch (no ``conf_matrix``, keyword ignored) behave as before"""
    m = _matcher(dev, sd, match_coarse={"thr": 1e-6})
    g = torch.Generator().manual_seed(11)
    views = torch.rand(3, 1, *VIEW, generator=g)
    query = torch.rand(1, 1, *QUERY, generator=g)
    query[0, 0, 16:16 + VIEW[0], 24:24 + VIEW[1]] = views[0, 0]
    data = {"image0": views.to(dev), "image1": query.to(dev)}
    eager, lazy = _run(m, data, None), _run(m, data, None, conf_matrix="lazy")
    K = _same_lists(lazy, eager, "real backbone")
    print(f"real backbone: K={K}")
    assert torch.equal(lazy["conf_matrix"].materialize(), eager["conf_matrix"])
    m.enable_fine_matching = False
    try:
        e2, l2 = _run(m, data, None), _run(m, data, None, conf_matrix="lazy")
    finally:
        m.enable_fine_matching = True
    for k in LISTS_EQUAL + ("mconf", "mkpts0_c", "mkpts1_c", "mkpts0_f", "mkpts1_f"):
        assert torch.equal(l2[k], e2[k]) and torch.equal(e2[k], eager[k] if not k.endswith("_f") else eager[k[:-1] + "c"]), k
    assert "expec_f" not in l2 and not isinstance(l2["conf_matrix"], torch.Tensor)
    one = {"image0": data["image0"][:1], "image1": data["image1"]}
    sel = eager["b_ids"] == 0
    given = {"mkpts0_c": eager["mkpts0_c"][sel].clone(), "mkpts1_c": eager["mkpts1_c"][sel].clone()}
    assert int(sel.sum()) > 0
    f_e, f_l = _run(m, {**one, **{k: v.clone() for k, v in given.items()}}, None), _run(m, {**one, **given}, None, conf_matrix="lazy")
    assert "conf_matrix" not in f_e and "conf_matrix" not in f_l
    for k in ("i_ids", "j_ids", "mconf", "expec_f", "mkpts0_f", "mkpts1_f"):
        assert torch.equal(f_e[k], f_l[k]), k


def test_lazy_call_does_not_allocate_the_matrix(matcher, dev):
    """peak allocated bytes, eager call minus lazy call on the same inputs, against the matrix's own size (10 % for the allocator's
    rounding).  V = 3 and a query of 192 x 256 (L1 = 768): 4 * 3 * 80 * 768 = 737 280 bytes, not lost in the rounding of small blocks.
    The peak statistics are reset before each call and once more at the backbone-output boundary (inside ``feature_hook``): over the
    whole call the peak is the backbone's (61 MB of activations at these sizes, freed before the coarse stage begins, the same in both
    forms -- whole-call peaks differ by 0), and the matrix lives from the coarse matching to the end of the fine stage"""
    V, hw1 = 3, (192, 256)
    L0, L1 = 80, 768
    planted = _planted_hook(dev, V, VIEW, hw1, shared=True)
    whole = {}

    def hook(fc0, ff0, fc1, ff1):
        torch.cuda.synchronize()
        whole["peak"] = torch.cuda.max_memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        return planted(None, None, None, None)
    data = _inputs(dev, V, VIEW, hw1, True, "plain")
    _run(matcher, data, planted), _run(matcher, data, planted, conf_matrix="lazy")          # packed weights and tables exist before measuring
    peaks = {}
    for form in ("eager", "lazy"):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        out = _run(matcher, data, hook, conf_matrix=form)
        torch.cuda.synchronize()
        peaks[form] = torch.cuda.max_memory_allocated()
        assert out["b_ids"].shape[0] > 0
        print(f"{form}: peak {peaks[form]} bytes after the backbone, {whole['peak']} in it; K = {out['b_ids'].shape[0]}")
        del out
    saved, matrix = peaks["eager"] - peaks["lazy"], 4 * V * L0 * L1
    print(f"saved {saved} bytes, the matrix has {matrix}")
    assert saved >= 0.9 * matrix


# ---- the tie re-run -----------------------------------------------------------------------------------------------------------------------
G0, G1 = (8, 10), (12, 16)                                          # the coarse grids of VIEW and QUERY
TIE_I, TIE_I2 = 3 * 10 + 4, 4 * 10 + 6                              # rows of image 0 (interior cells): the tied row and the one that beats it
TIE_J1, TIE_J2 = 5 * 16 + 6, 8 * 16 + 9                             # the two identical cells of image 1 (interior, J1 < J2)


def _tie_features(V, tie_pairs, seed=7):
    """final coarse rows for a matcher WITHOUT coarse layers (the planted rows are the matched rows): random background, a few plain
    matches per pair and, in ``tie_pairs``, the exact tie: cells J1 and J2 of image 1 carry the same row u, so columns J1 and J2 of the
    matrix are identical; row I of image 0 is 1.2 u -- its maximum is tied between J1 and J2 -- and row I2 is 1.21 u and beats it in
    both columns.  sim = <a, b> / 256 / 0.1 with |u|^2 = 256: 12 and 12.1 against a background of about +-0.6, so
    conf[I, J*] = 0.5 * 1 / (1 + e^0.1) = 0.24 > thr and conf[I2, J*] = 0.26"""
    g = torch.Generator().manual_seed(seed)
    L0, L1 = G0[0] * G0[1], G1[0] * G1[1]
    x0, x1 = torch.randn(V, L0, 256, generator=g), torch.randn(V, L1, 256, generator=g)
    for b in range(V):
        for n in range(6):                                          # plain matches: cell (2 + n % 4, 2 + n) of image 0 -> (3 + n, 3 + n) of image 1
            x1[b, (3 + n) * G1[1] + 3 + n] = x0[b, (2 + n % 4) * G0[1] + 2 + n]
        if b in tie_pairs:
            u = torch.randn(256, generator=g)
            u = u * (16.0 / u.norm())
            x1[b, TIE_J1] = u
            x1[b, TIE_J2] = u
            x0[b, TIE_I] = 1.2 * u
            x0[b, TIE_I2] = 1.21 * u
    fine = lambda hw: torch.randn(V, 16 * hw[0] * hw[1], 128, generator=g)
    return x0, fine(G0), x1, fine(G1)


@pytest.fixture(scope="module")
def flat_matcher(dev):
    """no coarse layers: ``feature_hook``'s rows reach the coarse matching as they are"""
    m = loftr.LoFTR_for_OnePose_Plus(dict(copy.deepcopy(loftr.default_cfg), coarse=dict(loftr.default_cfg["coarse"], layer_names=[]))).eval()
    m.load_state_dict(make_synthetic_loftr_state_dict(0, n_coarse=0), strict=True)
    return m.to(dev)


@pytest.mark.parametrize("V,tie_pairs,budget", [(1, (0,), None), (3, (1,), 0), (3, (1,), None), (3, (), 0)],
                         ids=["one_pair", "middle_pair_sub_batches", "middle_pair_one_rerun", "no_tie"])
def test_exact_tie_takes_the_eager_rerun(flat_matcher, dev, monkeypatch, V, tie_pairs, budget):
    m = flat_matcher
    feats = tuple(t.to(dev) for t in _tie_features(V, tie_pairs))
    hook = lambda fc0, ff0, fc1, ff1: feats
    data = _inputs(dev, V, VIEW, QUERY, False, "plain")
    eager = _run(m, data, hook)
    conf = eager["conf_matrix"]
    thr = m.config["match_coarse"]["thr"]
    for b in tie_pairs:                                             # the plant is what it claims to be
        assert torch.equal(conf[b, :, TIE_J1], conf[b, :, TIE_J2])
        assert float(conf[b, TIE_I].max()) == float(conf[b, TIE_I, TIE_J1]) > thr
        assert float(conf[b, TIE_I2, TIE_J1]) > float(conf[b, TIE_I, TIE_J1])
        got = {(bb, i): j for bb, i, j in zip(eager["b_ids"].tolist(), eager["i_ids"].tolist(), eager["j_ids"].tolist())}
        assert got[(b, TIE_I2)] == TIE_J1 and (b, TIE_I) not in got
    entered = []
    real_call = hip.call

    def spy(name, *args):
        if name.startswith("ophip_coarse_match_2d"):
            entered.append((name, args[4], args[13] is None))       # (entry, pairs, conf == NULL)
        return real_call(name, *args)
    monkeypatch.setattr(hip, "call", spy)
    before = m.lazy_reruns
    lazy = _run(m, data, hook, conf_matrix="lazy", budget_bytes=budget)
    monkeypatch.setattr(hip, "call", real_call)
    K = _same_lists(lazy, eager, (V, tie_pairs, budget))
    assert K >= 6 * V
    first = ("ophip_coarse_match_2d", V, True)
    if not tie_pairs:
        assert entered == [first] and m.lazy_reruns == before
    elif budget == 0:                                               # one-pair sub-batches, concatenated in pair order
        assert entered == [first] + [("ophip_coarse_match_2d", 1, False)] * V and m.lazy_reruns == before + 1
    else:
        assert entered == [first, ("ophip_coarse_match_2d", V, False)] and m.lazy_reruns == before + 1
    assert not isinstance(lazy["conf_matrix"], torch.Tensor) and torch.equal(lazy["conf_matrix"].materialize(), conf)
