"""GPU suite of the proposal filter: rpn_proposal_filter against its numpy restatement (tests/proposal_filter_ref.py), bit for
bit, and its composition with rpn_decode_nms through decode_and_nms and Proposer.  The oracle never decodes: where boxes matter it
is fed the device's own get_bboxes_from_deltas, or anchors whose decode is exact."""
import numpy as np
import pytest
import torch

import cases
import proposal_filter_ref as ref
from oracle import bbox_oracle as bo
from oracle import c_oracle as co
from tf_rpn_amd.utils import bbox_utils

pytestmark = pytest.mark.gpu

VAR = [0.1, 0.1, 0.2, 0.2]
NINF = float("-inf")


def _read(*tensors):
    """One device-to-host copy for several float32 / int32 tensors (moved as bit patterns)."""
    flat = torch.cat([t.contiguous().view(torch.int32).reshape(-1) for t in tensors]).cpu().numpy()
    out, off = [], 0
    for t in tensors:
        a = flat[off:off + t.numel()].reshape(tuple(t.shape))
        off += t.numel()
        out.append(a.view(np.float32) if t.dtype == torch.float32 else a)
    return out


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()          # (a copy: the shared fixtures are read-only)


def _same_bits(got, want):
    return np.array_equal(np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32))


SPECIALS = [np.nan, np.inf, -np.inf, 0.0, -0.0, -0.5, -1e-3, 1e-40, -1e-40, 2.0, 1e-45, 0.5]


def _scores(kind, A, seed):
    rng = np.random.RandomState(seed)
    if kind == "distinct":
        return cases.permutation_scores(rng, 3, A)
    if kind == "eighths":                                     # runs of ties: a cut always lands inside one
        return (np.floor(rng.uniform(0, 1, size=(3, A)) * 8) / 8).astype(np.float32)
    if kind == "equal":
        return np.full((3, A), 0.25, np.float32)
    s = cases.permutation_scores(rng, 3, A)                   # "special": NaN, +-inf, +-0.0, negatives, subnormals sprinkled in
    for b in range(3):
        n = min(A, len(SPECIALS))
        s[b, rng.choice(A, size=n, replace=False)] = np.array(SPECIALS, np.float32)[rng.permutation(len(SPECIALS))[:n]]
    return s


# ---- 1. top-N against the oracle --------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["distinct", "eighths", "equal", "special"])
@pytest.mark.parametrize("A", [1, 63, 64, 65, 1023, 1025, 8191, 8193, 8649])
def test_top_n_matches_the_oracle(A, kind):
    s = _scores(kind, A, seed=A)
    sd, anchors, deltas = _dev(s), torch.zeros((A, 4), device="cuda"), torch.zeros((3, A, 4), device="cuda")
    runs, outs = [], []
    for B in (1, 3):
        for N in sorted({n for n in (1, A // 3, A - 1, A, A + 5) if n >= 1}):
            for thr in (NINF, 0.0, 0.5):
                m, k = bbox_utils.filter_proposals(anchors, deltas[:B], sd[:B], VAR, pre_nms_topn=N, score_threshold=thr)
                runs.append((B, N, thr))
                outs += [m, k]
    host = _read(*outs)
    for i, (B, N, thr) in enumerate(runs):
        wm, wk = ref.filter_ref(None, s[:B], N, None, thr)
        assert np.array_equal(host[2 * i + 1], wk), (B, N, thr, host[2 * i + 1], wk)
        assert _same_bits(host[2 * i], wm), (B, N, thr)


@pytest.mark.parametrize("kind", ["distinct", "eighths"])
def test_top_n_at_61440_anchors(kind):
    A = 61440
    s = _scores(kind, A, seed=7)[:1]
    m, k = bbox_utils.filter_proposals(torch.zeros((A, 4), device="cuda"), torch.zeros((1, A, 4), device="cuda"), _dev(s), VAR,
                                       pre_nms_topn=6000)
    m, k = _read(m, k)
    wm, wk = ref.filter_ref(None, s, 6000)
    assert k.tolist() == wk.tolist() == [6000] and _same_bits(m, wm)


# ---- 2. minimum size, exact threshold ---------------------------------------------------------------
def test_min_size_exact_threshold():
    q = 1.0 / 64
    anchors = np.array([[16, 16, 24, 28],          # 0: h = 8/64, w = 12/64, inside the image
                        [-4, 8, 8, 40],            # 1: h = 12/64, 8/64 once clipped; w = 32/64
                        [8, 56, 40, 72],           # 2: w = 16/64, 8/64 once clipped; h = 32/64
                        [16, 16, 24, 28],          # 3: dh = +inf -> a NaN side
                        [16, 16, 24, 28],          # 4: dx = NaN -> NaN sides
                        [0, 0, 64, 64]], np.float32) * np.float32(q)
    A = len(anchors)
    deltas = np.zeros((1, A, 4), np.float32)       # expf(0) == 1: a decoded side IS the anchor's side
    deltas[0, 3, 2] = np.inf
    deltas[0, 4, 1] = np.nan
    scores = (0.5 + 0.01 * np.arange(A, dtype=np.float32))[None]
    h0, w0 = np.float32(8 * q), np.float32(12 * q)
    up = lambda v: float(np.nextafter(np.float32(v), np.float32(np.inf)))
    table = [  # (min_size, clip_boxes, kept rows)
        ((float(h0), 0.0), True, [1, 1, 1, 0, 0, 1]),              # a side equal to the minimum passes ...
        ((up(h0), 0.0), True, [0, 0, 1, 0, 0, 1]),                 # ... the next float32 above it does not
        ((0.0, float(w0)), True, [1, 1, 0, 0, 0, 1]),
        ((0.0, up(w0)), True, [0, 1, 0, 0, 0, 1]),
        ((12 * q, 0.0), True, [0, 0, 1, 0, 0, 1]),                 # row 1: the clipped height fails ...
        ((12 * q, 0.0), False, [0, 1, 1, 0, 0, 1]),                # ... the unclipped one passes
        ((up(12 * q), 0.0), False, [0, 0, 1, 0, 0, 1]),
        ((0.0, 16 * q), True, [0, 1, 0, 0, 0, 1]),                 # row 2 likewise in x
        ((0.0, 16 * q), False, [0, 1, 1, 0, 0, 1]),
        ((0.0, up(16 * q)), False, [0, 1, 0, 0, 0, 1]),
        (0.0, True, [1, 1, 1, 0, 0, 1]),                           # a NaN side fails even a minimum of 0
        (0.0, False, [1, 1, 1, 0, 0, 1]),
        (None, True, [1, 1, 1, 1, 1, 1]),                          # nothing is decoded: the same rows are kept
    ]
    ad, dd, sd = _dev(anchors), _dev(deltas), _dev(scores)
    outs = [bbox_utils.get_bboxes_from_deltas(ad, dd, variances=VAR)]
    for min_size, clip, _want in table:
        outs += list(bbox_utils.filter_proposals(ad, dd, sd, VAR, min_size=min_size, clip_boxes=clip))
    host = _read(*outs)
    boxes = host[0]
    assert np.array_equal(boxes[0, [0, 1, 2, 5]], anchors[[0, 1, 2, 5]])          # the premise: zero deltas decode exactly
    for i, (min_size, clip, want) in enumerate(table):
        m, k = host[1 + 2 * i], host[2 + 2 * i]
        want_m = np.where(np.array(want, bool), scores[0], np.float32(NINF)).astype(np.float32)[None]
        assert _same_bits(m, want_m), (min_size, clip, m)
        assert k.tolist() == [sum(want)]
        om, ok = ref.filter_ref(boxes if min_size is not None else None, scores, None, min_size, NINF, clip)
        assert _same_bits(om, want_m) and ok.tolist() == k.tolist(), (min_size, clip)


# ---- 3. minimum size on random inputs ---------------------------------------------------------------
@pytest.fixture(scope="module")
def vgg_case():
    """VGG16's anchor grid (A = 8649), deltas ~ N(0, 0.5), the device's own decode of them, uniform scores."""
    hp = bo.get_hyper_params("vgg16")
    anchors = bo.generate_anchors(hp)
    rng = np.random.RandomState(5)
    deltas = (rng.standard_normal((2, len(anchors), 4)) * 0.5).astype(np.float32)
    scores = rng.uniform(0, 1, size=(2, len(anchors))).astype(np.float32)
    boxes = bbox_utils.get_bboxes_from_deltas(anchors, deltas, variances=VAR)
    for a in (anchors, deltas, scores, boxes):
        a.setflags(write=False)
    return anchors, deltas, scores, boxes


MIN_SIZE = 0.25       # a quarter of the image side: about a third of the decoded anchors are smaller (checked below)


def test_min_size_on_random_deltas(vgg_case):
    anchors, deltas, scores, boxes = vgg_case
    assert len(anchors) == 8649
    for clip in (True, False):
        fail = 1.0 - ref.size_ok(boxes, MIN_SIZE, clip).mean()
        assert 0.05 <= fail <= 0.95, fail                           # the size test is not vacuous on this input
    ad, dd, sd = _dev(anchors), _dev(deltas), _dev(scores)
    runs = [(None, MIN_SIZE, NINF, True), (2000, MIN_SIZE, NINF, True), (2000, (MIN_SIZE, 0.1), 0.3, False),
            (8000, (0.0, MIN_SIZE), NINF, True)]
    outs = []
    for N, m, thr, clip in runs:
        outs += list(bbox_utils.filter_proposals(ad, dd, sd, VAR, pre_nms_topn=N, min_size=m, score_threshold=thr, clip_boxes=clip))
    host = _read(*outs)
    for i, (N, m, thr, clip) in enumerate(runs):
        wm, wk = ref.filter_ref(boxes, scores, N, m, thr, clip)
        assert np.array_equal(host[2 * i + 1], wk), (N, m, thr, clip, host[2 * i + 1], wk)
        assert _same_bits(host[2 * i], wm), (N, m, thr, clip)
    # the size test comes first and the cut counts the survivors: the 2000 kept are the best 2000 of the boxes that pass
    wm, wk = ref.filter_ref(boxes, scores, 2000, MIN_SIZE)
    assert wk.tolist() == [2000, 2000]
    assert not np.array_equal(wm, ref.filter_ref(None, scores, 2000)[0])


# ---- 4. composition with the NMS --------------------------------------------------------------------
def _compose(anchors, deltas, scores, boxes, M, N, m):
    masked_ref, _ = ref.filter_ref(boxes, scores, N, m)
    ad, dd = _dev(anchors), _dev(deltas)
    got = bbox_utils.decode_and_nms(ad, dd, _dev(scores), VAR, M, iou_threshold=0.7, pre_nms_topn=N, min_size=m)
    want = bbox_utils.decode_and_nms(ad, dd, _dev(masked_ref), VAR, M, iou_threshold=0.7)
    host = _read(*(got + want))
    for g, w in zip(host[:4], host[4:]):
        assert _same_bits(g, w) if g.dtype == np.float32 else np.array_equal(g, w)
    _b, _s, idx, valid = host[:4]
    _rb, _rs, _rc, rv, ri = co.combined_nms(boxes[:, :, None, :], masked_ref[:, :, None], M, M, iou_threshold=0.7)
    assert np.array_equal(valid, rv), (valid, rv)
    assert np.array_equal(idx, ri)
    return valid


@pytest.mark.parametrize("M", [300, 2000])
def test_composition_equals_nms_of_the_masked_scores(vgg_case, M):
    anchors, deltas, scores, boxes = vgg_case
    valid = _compose(anchors, deltas, scores, boxes, M, 3000, MIN_SIZE)
    assert (valid > 0).all()


def test_composition_at_61440_anchors():
    """One image with 61440 anchors: the NMS behind the filter takes its several-workgroups-per-image path."""
    hp = bo.get_hyper_params("mobilenet_v2", img_size=1024, feature_map_shape=64, anchor_ratios=[1., 2., .5, 3., 1 / 3.])
    anchors = bo.generate_anchors(hp)
    A = len(anchors)
    assert A == 61440
    rng = np.random.RandomState(6)
    deltas = (rng.standard_normal((1, A, 4)) * 0.5).astype(np.float32)
    scores = rng.uniform(0, 1, size=(1, A)).astype(np.float32)
    boxes = bbox_utils.get_bboxes_from_deltas(anchors, deltas, variances=VAR)
    fail = 1.0 - ref.size_ok(boxes, 0.1).mean()
    assert 0.05 <= fail <= 0.95, fail
    valid = _compose(anchors, deltas, scores, boxes, 300, 6000, 0.1)
    assert valid.tolist() == [300]


# ---- 5. nothing changes by default ------------------------------------------------------------------
def test_defaults_leave_decode_and_nms_unchanged(vgg_case):
    anchors, deltas, scores, _boxes = vgg_case
    ad, dd, sd = _dev(anchors), _dev(deltas), _dev(scores)
    A = len(anchors)
    plain = bbox_utils.decode_and_nms(ad, dd, sd, VAR, 300, iou_threshold=0.7)
    none = bbox_utils.decode_and_nms(ad, dd, sd, VAR, 300, iou_threshold=0.7, pre_nms_topn=None, min_size=None)
    full = bbox_utils.decode_and_nms(ad, dd, sd, VAR, 300, iou_threshold=0.7, pre_nms_topn=A, min_size=None)
    more = bbox_utils.decode_and_nms(ad, dd, sd, VAR, 300, iou_threshold=0.7, pre_nms_topn=A + 1000)
    host = _read(*(plain + none + full + more))
    for j in range(4, 16):
        assert np.array_equal(host[j].view(np.uint32), host[j % 4].view(np.uint32)), j
    assert (host[3] == 300).all()


@pytest.fixture(scope="module")
def small_model():
    """smoke()'s model: VGG16 at img_size 96, feature map 6 (A = 324), synthetic weights, two batches of two images."""
    from tf_rpn_amd.models._rpn_model import synthetic_weights
    hp = bo.get_hyper_params("vgg16", img_size=96, feature_map_shape=6)
    weights = synthetic_weights("vgg16", hp, seed=1)
    rng = np.random.RandomState(0)
    xs = [_dev(rng.uniform(0, 1, size=(2, 96, 96, 3)).astype(np.float32)) for _ in range(2)]
    return hp, weights, xs


def _proposer(small_model, **kwargs):
    from tf_rpn_amd.predictor import Proposer
    hp, weights, _xs = small_model
    return Proposer("vgg16", hyper_params=dict(hp), weights=weights, precision="f32", max_batch=2, iou_threshold=0.7, **kwargs)


def test_default_proposer_equals_plain_decode_and_nms(small_model):
    prop = _proposer(small_model)
    assert prop._filter is None and not hasattr(prop, "_masked")
    x = small_model[2][0]
    boxes, scores, valid, idx = (t.clone() for t in prop.propose(x))
    deltas, obj = prop.forward(x)
    want = bbox_utils.decode_and_nms(prop.anchors, deltas, obj, prop.variances, prop.topn, iou_threshold=0.7)
    host = _read(boxes, scores, idx, valid, *want)
    for g, w in zip(host[:4], host[4:]):
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32))
    assert (host[3] > 0).all()


# ---- 6. Proposer ------------------------------------------------------------------------------------
FILTER = dict(pre_nms_topn=100, min_size=8 / 96)


def test_proposer_runs_the_filter_in_front_of_the_nms(small_model):
    prop = _proposer(small_model, **FILTER)
    assert tuple(prop._masked.shape) == (2, prop.total_anchors) and prop.total_anchors == 324
    x = small_model[2][0]
    boxes, scores, valid, idx = (t.clone() for t in prop.propose(x))
    deltas, obj = prop.forward(x)
    want = bbox_utils.decode_and_nms(prop.anchors, deltas, obj, prop.variances, prop.topn, iou_threshold=0.7, **FILTER)
    _m, kept = bbox_utils.filter_proposals(prop.anchors, deltas, obj, prop.variances, **FILTER)
    host = _read(boxes, scores, idx, valid, *want, kept)
    for g, w in zip(host[:4], host[4:8]):
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32))
    assert (host[3] > 0).all() and (host[3] <= host[8]).all() and (host[8] <= 100).all()


def test_proposer_overlap_nms_gives_the_same_bits(small_model):
    xs = small_model[2]
    plain = _proposer(small_model, **FILTER)
    piped = _proposer(small_model, overlap_nms=True, **FILTER)
    outs = []
    for prop in (plain, piped):
        for x in xs:                                                  # two consecutive batches: both buffer slots
            outs += [t.clone() for t in prop.propose(x)]
    host = _read(*outs)
    for j in range(8):
        assert np.array_equal(host[j].view(np.uint32), host[8 + j].view(np.uint32)), j
    assert (host[2] > 0).all()


def test_propose_features_pools_under_the_filtered_proposals(small_model):
    prop = _proposer(small_model, **FILTER)
    x = small_model[2][1]
    pb, ps, pv, _pi = (t.clone() for t in prop.propose(x))
    fb, fs, fv, pooled = prop.propose_features(x)
    want_pooled = prop.feature_extractor.roi_pool(fb, (7, 7), valid=fv)
    host = _read(pb, ps, pv, fb, fs, fv, pooled, want_pooled)
    for j in range(3):
        assert np.array_equal(host[j].view(np.uint32), host[3 + j].view(np.uint32)), j
    assert np.array_equal(host[6].view(np.uint32), host[7].view(np.uint32))
    assert np.abs(host[6]).max() > 0


# ---- 7. edges and determinism -----------------------------------------------------------------------
def test_a_minimum_nothing_reaches_drops_everything(vgg_case):
    anchors, deltas, scores, _boxes = vgg_case
    ad, dd, sd = _dev(anchors), _dev(deltas), _dev(scores)
    m, kept = bbox_utils.filter_proposals(ad, dd, sd, VAR, min_size=(2, 2))
    boxes, sc, idx, valid = bbox_utils.decode_and_nms(ad, dd, sd, VAR, 300, iou_threshold=0.7, min_size=(2, 2))
    m, kept, boxes, sc, idx, valid = _read(m, kept, boxes, sc, idx, valid)
    assert np.isneginf(m).all() and kept.tolist() == [0, 0] and valid.tolist() == [0, 0]
    assert not boxes.view(np.uint32).any() and not sc.view(np.uint32).any() and (idx == -1).all()


def test_an_all_nan_image_keeps_nothing_and_leaves_its_neighbours_alone():
    A = 1025
    s = _scores("eighths", A, seed=3)
    s[1] = np.nan
    anchors, deltas = torch.zeros((A, 4), device="cuda"), torch.zeros((3, A, 4), device="cuda")
    m, k = _read(*bbox_utils.filter_proposals(anchors, deltas, _dev(s), VAR, pre_nms_topn=200))
    wm, wk = ref.filter_ref(None, s, 200)
    assert k.tolist() == wk.tolist() == [200, 0, 200] and _same_bits(m, wm) and np.isneginf(m[1]).all()


def test_two_runs_and_single_images_give_the_same_bits(vgg_case):
    anchors, deltas, scores, _boxes = vgg_case
    rng = np.random.RandomState(9)
    d3 = np.concatenate([deltas, deltas[:1][:, ::-1]], axis=0)
    s3 = (np.floor(rng.uniform(0, 1, size=(3, len(anchors))) * 64) / 64).astype(np.float32)        # ties across the cut
    ad, dd, sd = _dev(anchors), _dev(d3), _dev(s3)
    kw = dict(pre_nms_topn=1500, min_size=MIN_SIZE)
    outs = list(bbox_utils.filter_proposals(ad, dd, sd, VAR, **kw)) + list(bbox_utils.filter_proposals(ad, dd, sd, VAR, **kw))
    for b in range(3):
        outs += list(bbox_utils.filter_proposals(ad, dd[b:b + 1], sd[b:b + 1], VAR, **kw))
    host = _read(*outs)
    m, k = host[0], host[1]
    assert _same_bits(host[2], m) and np.array_equal(host[3], k)
    for b in range(3):
        assert _same_bits(host[4 + 2 * b][0], m[b]) and host[5 + 2 * b][0] == k[b], b
    assert k.tolist() == [1500, 1500, 1500]
