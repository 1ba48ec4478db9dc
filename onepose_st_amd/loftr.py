"""``LoFTR_for_OnePose_Plus`` -- the 2D-2D matcher behind the object detector on the HIP kernels.

Mirrors the interface of ``src/KeypointFreeSfM/loftr_for_sfm/loftr.py:16-167``: ``LoFTR_for_OnePose_Plus(config,
enable_fine_matching=True)``, ``state_dict`` keys ``backbone.*`` / ``loftr_coarse.layers.{0..7}.*`` / ``loftr_fine.layers.{0,1}.*``
(what ``build_2D_match_model`` loads with ``strict=True``, ``local_feature_2D_detector.py:24-37``), ``forward(data)`` mutating
``data`` (``image0``, ``image1`` in; ``hw*_i/c/f``, ``b_ids``, ``i_ids``, ``j_ids``, ``mconf``, ``mkpts0_c``, ``mkpts1_c``,
``expec_f``, ``mkpts0_f``, ``mkpts1_f``, ``conf_matrix`` out).  ``default_cfg`` restates ``loftr_for_onepose_plus_cfg.py:10-50``.

The reference imports the arithmetic from ``submodules/LoFTR`` (un-vendored): it is taken here from the published zju3dv/LoFTR
definition (``oracle/loftr_oracle.py`` restates it on the CPU; parity unpinned).  Kernels:

* backbone ``ResNetFPN_8_2``: ``backbone_hip.HipBackbone`` (``ophip_conv2d_bf16``), positional encoding in the last epilogue;
* 8 coarse layers ``[self, cross] x 4``: ``ophip_encoder_layer_x3w8``.  LoFTR's ``cross`` is sequential (image 1 attends to the
  UPDATED image 0), so a cross layer is two ONE-stream launches (``ophip_encoder_layer_x3w8_streams``): image 0's rows against image 1,
  then image 1's rows against the new image 0 (rounds 3-4 ran the two-stream kernel twice and discarded half of each result);
* batch: ``image0 [V, 1, H, W]`` against ``image1 [1 or V, 1, H, W]`` in ONE call -- the detector's ~15 reference views against one query
  frame (the query's backbone features are computed once); ``b_ids`` names the pair of every match;
* dual-softmax + mutual-nearest between the two grids: ``ophip_coarse_match_2d`` (temperature exactly 0.1, all-sides border);
* fine stage, window 9 on both images, batched over all matches: ``csrc/loftr_fine.hip``.  ``fine_window_size`` is odd, from 3 to 11
  (``ValueError`` at construction otherwise).

``coarse.attention`` / ``fine.attention`` = ``"full"`` (each on its own; the reference config's other option) swap the attention form
(``FullAttention``, same ``state_dict``): a coarse layer is then ``ophip_encoder_layer_full_x3_stream`` (one query stream per launch,
the f32 layer block), a shared query image is passed with batch stride 0 instead of being copied V times and its layer-0 self layer runs
once; the fine layers call ``ophip_fine2_full_attention`` (W x W windows, softmax) in place of the linear attention.

``match_coarse.match_type`` = ``"sinkhorn"`` (the config's other option) swaps the dual softmax for optimal transport with a dustbin
(LoFTR's ``CoarseMatching`` sinkhorn branch, SuperGlue's ``log_optimal_transport``, ``skh_iters`` iterations, ``skh_prefilter``):
``ophip_coarse_match_2d_sinkhorn``.  Such a model has one more parameter, ``coarse_matching.bin_score`` (0-d, ``skh_init_bin_score``).

The SfM calls (``loftr_for_sfm/loftr.py:79-167``):

* ``scale0`` / ``scale1`` (float32 ``[V, 2]``, ``scale1`` also ``[1, 2]`` when ``image1`` has batch 1; the reference's [h, w] factors,
  applied as given on the coarse path and in FineMatching): ``mkpts*_c`` times ``scale[b]`` on the device, ``ophip_fine2_match_scaled``;
* provided coarse matches ``mkpts0_c`` / ``mkpts1_c`` (float32 / float64 ``[K, 2]``, one pair): the fine-only branch --
  ``ophip_loftr_coarse_ids`` clips the caller's tensors in place and rounds them to cells (``IndexError`` for an id past the grid when
  the fine stage runs), no coarse transformer, ``mconf`` int64 ones, no ``conf_matrix``;
* ``extract_coarse_feature`` / ``extract_fine_feature``: ``feat_coarse_b_{0,1} [K, 256]`` (nearest) and ``feat_ext{0,1} [K, 128]``
  (bilinear) sampled from the backbone maps before the positional encoding at ``mkpts*_f``, one ``ophip_sample_features`` launch.

Padding masks ``mask0`` / ``mask1`` (``loftr_for_sfm/loftr.py:38-42, 72-78``): ``torch.bool`` ``[V, h0c, w0c]`` and
``[V1, h1c, w1c]`` at coarse resolution (``True`` = a real cell; ``V1`` = image1's batch, a batch-1 ``mask1`` is repeated for every pair),
on the device, both or neither.  They mask both streams of every coarse layer (``ophip_encoder_layer_x3w8_masks`` /
``ophip_encoder_layer_x3w8_streams_masks``: phi(K), V of padded source rows and phi(Q) of padded query rows are zero, ``v_length`` stays
the padded length), fill the similarity with -1e9 where either cell is padding and take the border from each pair's valid extent
(``ophip_coarse_match_2d_masked`` / ``ophip_coarse_match_2d_sinkhorn_masked``, ``mask_border_with_padding``).  The fine stage, the
scales, extraction and the fine-only branch (which ignores them, as the reference does) are unchanged.  With ``coarse.attention =
"full"`` masks raise: the published ``FullAttention`` fills a padded query row with -inf, its softmax is NaN, and the NaN reaches every
row one layer later.

``config["hip_conf_matrix"]`` = ``"lazy"`` (this build's key; ``"eager"`` when absent), or ``forward(data, conf_matrix="lazy")`` for one
call: the ``[V, L0, L1]`` matrix is not stored -- ``ophip_coarse_match_2d[_masked]`` with ``conf == NULL``; every
match list equals the eager form's bit for bit -- and ``data["conf_matrix"]`` is a :class:`LazyConfMatrix` that computes it on first
use.  An exact row tie that the lazy selection cannot resolve (``count[1]``, read with the match count in one copy) runs the coarse
matching again eagerly on the same final rows; ``lazy_reruns`` counts those calls, ``forward(..., budget_bytes=n)`` splits the re-run into
sub-batches of pairs within ``n`` bytes (:meth:`LoFTR_for_OnePose_Plus.coarse_batch_bytes`).  Sinkhorn matching needs the matrix:
``"lazy"`` with it is a ``ValueError``, as is any other value.

``fine_concat_coarse_feat`` = ``True`` (LoFTR's published setting): the model owns ``fine_preprocess.down_proj`` and
``fine_preprocess.merge_feat`` (``Linear(256, 128)`` with bias each, also with ``enable_fine_matching=False``: the public checkpoints load
strictly), and between the window gather and the fine transformer every window row becomes ``merge_feat(cat[row, down_proj(coarse row of
its match)])`` on both images: ``fine_context.merge`` (``opfcx_merge`` of ``libonepose_fine_context.so``), in place, on the coarse
transformer's final rows.  The fine-only branch has no such rows and raises, as does ``sfm_fine``.

Malformed masks (a lone mask, another dtype, image-resolution masks, a wrong batch or grid), malformed scale / keypoint tensors, a tensor
without its partner, V > 1 with provided matches or extraction, and coarse extraction with a ``feature_hook`` raise
``NotImplementedError`` before anything runs.  No CPU fallback.
"""
from __future__ import annotations

import copy
import ctypes

import torch
import torch.nn as nn

from . import fine_context, hip, host_math, layercall, packing
from .backbone import build_backbone
from .backbone_hip import HipBackbone, pack_backbone
from .lazy_conf import LazyConfMatrixBase
from .matchcall import MatchLists, coarse_match_2d
from .params import EncoderParams, load_matcher_checkpoint
from .rows import rows_encoder_layer

# this build's own config keys and their defaults.  "hip_conf_matrix": "eager" stores conf_matrix, "lazy" does not (see the module text)
BUILD_KEYS = {"hip_conf_matrix": "eager"}
# what the fine-only branch (and sfm_fine, which is built on it) says of a matcher with fine_concat_coarse_feat
FINE_ONLY_WITH_CONTEXT = ("fine_concat_coarse_feat with provided coarse matches: the fine windows take their context from the coarse "
                          "transformer's output, which the fine-only branch does not compute (the published class fails there too)")


class _ReferenceConfig(dict):
    """``default_cfg``: its items are the reference's config and nothing else -- it still compares equal to the reference's dict -- and
    a lookup of one of this build's own keys (``BUILD_KEYS``) answers with that key's default.  A config that sets such a key holds it
    as an ordinary item; one without it (any plain dict written for the reference) means the default."""

    def __missing__(self, key):
        return BUILD_KEYS[key]


default_cfg = _ReferenceConfig({
    "backbone_type": "ResNetFPN", "resolution": (8, 2), "fine_window_size": 9, "fine_concat_coarse_feat": False,
    "resnetfpn": {"initial_dim": 128, "block_dims": [128, 196, 256]},
    "coarse": {"d_model": 256, "d_ffn": 256, "nhead": 8, "layer_names": ["self", "cross"] * 4, "attention": "linear", "temp_bug_fix": False},
    "match_coarse": {"thr": 0.2, "border_rm": 2, "match_type": "dual_softmax", "dsmax_temperature": 0.1, "skh_iters": 3,
                     "skh_init_bin_score": 1.0, "skh_prefilter": True, "train_coarse_percent": 0.4, "train_pad_num_gt_min": 200},
    "fine": {"d_model": 128, "d_ffn": 128, "nhead": 8, "layer_names": ["self", "cross"] * 1, "attention": "linear"},
})


class LazyConfMatrix(LazyConfMatrixBase):
    """``data["conf_matrix"]`` of a lazy call: keeps the coarse transformer's final rows ``x0 [V, L0, 256]``, ``x1 [V, L1, 256]`` (and the
    flattened padding masks) and nothing V x L0 x L1.  First use runs ``match(x0, x1, masks)`` -- the eager
    ``ophip_coarse_match_2d[_masked]`` call on those rows with scratch match lists -- and keeps its matrix: the eager forward's bits."""

    def __init__(self, match, x0, x1, masks, stream):
        super().__init__((x0.shape[0], x0.shape[1], x1.shape[1]), x0.device)
        self._match, self._x0, self._x1, self._masks, self._stream = match, x0, x1, masks, stream

    def _compute(self) -> torch.Tensor:
        torch.cuda.current_stream(self.device).wait_stream(self._stream)          # the forward's stream has produced the rows
        conf = self._match(self._x0, self._x1, self._masks)
        self._match = self._x0 = self._x1 = self._masks = None
        return conf


class LoFTR_for_OnePose_Plus(nn.Module):
    def __init__(self, config=None, enable_fine_matching=True):
        super().__init__()
        config = copy.deepcopy(default_cfg) if config is None else config
        self.config = config
        self.enable_fine_matching = enable_fine_matching
        if config["backbone_type"] != "ResNetFPN" or tuple(config["resolution"]) != (8, 2):
            raise NotImplementedError("LoFTR backbone: ResNetFPN 8 -> 2 only")
        cc, cf, mc = config["coarse"], config["fine"], config["match_coarse"]
        if cc["d_model"] != 256 or cc["nhead"] != 8 or cf["d_model"] != 128 or cf["nhead"] != 8:
            raise NotImplementedError("HIP kernels are specialised for d_model 256 / 128 with 8 heads")
        for enc, c in (("coarse", cc), ("fine", cf)):
            if c["attention"] not in ("linear", "full"):
                raise NotImplementedError(f"{enc}.attention: linear or full")
        self.coarse_full, self.fine_full = cc["attention"] == "full", cf["attention"] == "full"
        if mc["match_type"] not in ("dual_softmax", "sinkhorn"):
            raise NotImplementedError("match_coarse.match_type: dual_softmax or sinkhorn")
        self.sinkhorn = mc["match_type"] == "sinkhorn"
        # "lazy": conf_matrix is not stored (ophip_coarse_match_2d[_masked] with conf == NULL; the match lists are the eager form's bit
        # for bit) and data["conf_matrix"] is a LazyConfMatrix.  forward(data, conf_matrix=...) overrides it for one call
        self.conf_matrix_mode = self._conf_form(config.get("hip_conf_matrix", BUILD_KEYS["hip_conf_matrix"]), "hip_conf_matrix")
        self.lazy_reruns = 0                           # lazy calls that met an exact row tie and ran the coarse matching again eagerly
        if self.sinkhorn:
            iters = mc["skh_iters"]
            if isinstance(iters, bool) or not isinstance(iters, int) or iters < 0:
                raise ValueError("match_coarse.skh_iters: an int >= 0")
            if mc.get("sparse_spvs", False):
                raise NotImplementedError("match_coarse.sparse_spvs: training output (conf_matrix_with_bin)")
        if cc["temp_bug_fix"]:
            raise NotImplementedError("temp_bug_fix: the reference's detector config runs the original (floor-division) position table")
        self.fine_context = bool(config["fine_concat_coarse_feat"])
        W = int(config["fine_window_size"])
        if W < 3 or W % 2 == 0 or W * W > 128:             # FineMatching's grid step is 2 / (W - 1); W * W heat-map slots <= 128
            raise ValueError("fine_window_size must be odd, from 3 to 11")
        for n in list(cc["layer_names"]) + list(cf["layer_names"]):
            if n not in ("self", "cross"):
                raise KeyError(n)
        self.backbone = build_backbone({"type": "ResNetFPN", "resolution": [8, 2],
                                        "resnetfpn": {"block_type": "BasicBlock", "initial_dim": config["resnetfpn"]["initial_dim"],
                                                      "block_dims": list(config["resnetfpn"]["block_dims"]), "output_layers": [3, 1]}})
        self.loftr_coarse = EncoderParams(cc["layer_names"], cc["d_model"], cc["nhead"])
        self.loftr_fine = EncoderParams(cf["layer_names"], cf["d_model"], cf["nhead"])
        if self.fine_context:                          # the published FinePreprocess holds them whether or not the fine stage runs
            self.fine_preprocess = nn.Module()
            self.fine_preprocess.down_proj = nn.Linear(cc["d_model"], cf["d_model"], bias=True)
            self.fine_preprocess.merge_feat = nn.Linear(2 * cf["d_model"], cf["d_model"], bias=True)
        if self.sinkhorn:                              # the reference's CoarseMatching holds bin_score in the sinkhorn form only
            self.coarse_matching = nn.Module()
            self.coarse_matching.bin_score = nn.Parameter(torch.tensor(float(mc["skh_init_bin_score"]), requires_grad=True))
        self._packed = None
        self._pe = {}
        # optional ``hook(fc0 [1, L0, 256], ff0 [hf0 * wf0, 128], fc1, ff1) -> the same four``: the backbone-output boundary (coarse rows
        # with the positional encoding added, fine maps channels-last) -- the counterpart of a forward hook on the reference's backbone.
        # (a batched call hands it ``fc0 [V, L0, 256], ff0 [V, hf0 * wf0, 128], fc1 [1 or V, ...], ff1`` and takes the same back)
        self.feature_hook = None

    # ------------------------------------------------------------------------------------------
    def _conf_form(self, value, what) -> str:
        """``"eager"`` / ``"lazy"`` -> the value; anything else, or ``"lazy"`` with sinkhorn matching, raises ``ValueError``"""
        if value not in ("eager", "lazy"):
            raise ValueError(f"{what} {value!r}: expected 'eager' or 'lazy'")
        if value == "lazy" and self.sinkhorn:
            raise ValueError(f"{what} = 'lazy' with match_type 'sinkhorn': ophip_coarse_match_2d_sinkhorn requires conf")
        return value

    def coarse_batch_bytes(self, V: int, hw0_c, hw1_c, lazy: bool) -> int:
        """Upper estimate, in bytes, of what the coarse stage of ONE call allocates for ``V`` pairs of coarse grids ``hw0_c`` x ``hw1_c``
        (cells): what :class:`onepose_st_amd.detector.LocalFeatureObjectDetector` holds against its ``batch_budget_bytes``.  The sum of

        * ``4 * V * (L0 + L1) * 256 * 4``: the rows -- input, output and one layer in flight for both streams, the shared query expanded;
        * the coarse transformer's workspace: ``ophip_encoder_x3w8_workspace_bytes(V, L0, L1)``, with ``coarse.attention = "full"``
          ``ophip_encoder_full_stream_workspace_bytes(V, max(L0, L1), max(L0, L1))``;
        * the coarse matching's workspace: ``4 * ophip_coarse_workspace_floats(V, L0, L1)`` (sinkhorn: its own query);
        * the match lists of capacity ``V * L0``: 57 bytes a slot as the entry point writes them, 24 more for their compacted and scaled
          copies, and 64 bytes a cell of image 0 plus 8 KiB for the point table, the count and the allocator's rounding of small blocks;
        * ``4 * V * L0 * L1`` for ``conf_matrix`` when not ``lazy``.

        Host arithmetic and three size queries: no device is touched.  Not counted: the backbone, and the fine stage's buffers
        (``K * W * W * 128`` floats, a few at a time), which depend on the number of matches; the eager re-run of a lazy call that met an
        exact tie (it is held under the budget by its own sub-batches)."""
        lib = hip.load()
        V, L0, L1 = int(V), int(hw0_c[0]) * int(hw0_c[1]), int(hw1_c[0]) * int(hw1_c[1])
        rows = 4 * V * (L0 + L1) * 256 * 4
        Lm = max(L0, L1)
        enc = layercall.workspace_bytes("full", V, Lm, Lm, stream_form=True) if self.coarse_full else layercall.workspace_bytes("bf16x3", V, L0, L1)
        cws = 4 * (lib.ophip_coarse_sinkhorn_workspace_floats if self.sinkhorn else lib.ophip_coarse_workspace_floats)(V, L0, L1)
        lists = (57 + 24) * V * L0 + 64 * L0 + 8192
        return int(rows + enc + cws + lists + (0 if lazy else 4 * V * L0 * L1))

    def _blocks(self, device):
        params = list(self.parameters()) + list(self.buffers())
        key = (str(device),) + tuple((p.data_ptr(), p._version) for p in params)
        if self._packed is None or self._packed[0] != key:
            sd = self.state_dict()
            bb = {k[len("backbone."):]: v for k, v in sd.items() if k.startswith("backbone.")}
            self._packed = (key, {
                "backbone": pack_backbone(bb, device),
                "coarse": [(packing.pack_coarse_layer if self.coarse_full else packing.pack_coarse_layer_x3w8)(sd, f"loftr_coarse.layers.{i}.").to(device)
                           for i in range(len(self.loftr_coarse.layer_names))],
                "fine": [{n: t.to(device) for n, t in packing.pack_fine_layer_full_x3(sd, f"loftr_fine.layers.{i}.").items()}
                         for i in range(len(self.loftr_fine.layer_names))],
                "bin_score": float(sd["coarse_matching.bin_score"]) if self.sinkhorn else None,
                "context": packing.pack_fine_context(sd).to(device) if self.fine_context else None,
            })
        return self._packed[1]

    def _pe_table(self, h, w, device):
        k = (h, w, str(device))
        if k not in self._pe:
            self._pe[k] = host_math.pe_table(self.config["coarse"]["d_model"], h, w, (256, 256)).to(device)      # the floor-division table (temp_bug_fix False)
        return self._pe[k]

    # ------------------------------------------------------------------------------------------
    def _coarse_linear(self, Wc, fc0, fc1, shared1, V, L0, L1, masks=None):
        """``masks``: None or the flattened padding masks ``(m0 [V, L0], m1 [V, L1])`` (bool, contiguous; a shared query's mask already
        repeated with its rows)"""
        x0 = fc0.contiguous()
        x1 = (fc1.expand(V, -1, -1) if shared1 else fc1).contiguous()
        fixed = dict(mode="bf16x3", workspace=layercall.workspace("bf16x3", V, L0, L1, x0.device), masks=masks)
        for w, name in zip(Wc, self.loftr_coarse.layer_names):
            if name == "self":
                b0, b1 = torch.empty_like(x0), torch.empty_like(x1)
                layercall.layer(x0, x1, b0, b1, wpack=w, is_cross=0, **fixed)
                x0, x1 = b0, b1
            else:
                n0 = torch.empty_like(x0)              # image 0 against image 1
                layercall.layer(x0, x1, n0, None, wpack=w, is_cross=1, streams=1, **fixed)
                n1 = torch.empty_like(x1)              # image 1 against the UPDATED image 0
                layercall.layer(n0, x1, None, n1, wpack=w, is_cross=1, streams=2, **fixed)
                x0, x1 = n0, n1
        return x0, x1

    def _coarse_full(self, Wc, x0, x1, V, L0, L1):
        """full attention, one query stream per launch; ``x1 [1, L1, 256]`` against ``x0 [V, L0, 256]`` is one query image shared by the
        V pairs: it is read with batch stride 0 (projected once) until the first cross layer gives every pair its own rows, and a self
        layer before that runs on it once"""
        Lm = max(L0, L1)
        ws = layercall.workspace("full", V, Lm, Lm, x0.device, stream_form=True)

        def layer(x, src, w):
            y = torch.empty(max(x.shape[0], src.shape[0]), x.shape[1], 256, device=x.device)
            layercall.layer_full_stream(x, src, y, wpack=w, workspace=ws)
            return y
        for w, name in zip(Wc, self.loftr_coarse.layer_names):
            if name == "self":
                x0, x1 = layer(x0, x0, w), layer(x1, x1, w)
            else:
                x0 = layer(x0, x1, w)                  # image 0 against image 1
                x1 = layer(x1, x0, w)                  # image 1 against the UPDATED image 0
        if x1.shape[0] != V:                           # no cross layer: the query's rows are still shared
            x1 = x1.expand(V, -1, -1).contiguous()
        return x0, x1

    def _check_inputs(self, data, kwargs):
        """the input forms outside what the kernels cover raise before anything runs; -> (fine_only, has_scales, extract_c, extract_f)"""
        V, V1 = data["image0"].size(0), data["image1"].size(0)
        has_m = "mask0" in data
        if has_m != ("mask1" in data):
            raise NotImplementedError("'mask0' and 'mask1' come together")
        if has_m:
            for k, img, rows in (("mask0", data["image0"], V), ("mask1", data["image1"], V1)):
                t = data[k]
                grid = (rows, img.shape[2] // 8, img.shape[3] // 8)
                if not isinstance(t, torch.Tensor) or t.dtype != torch.bool or tuple(t.shape) != grid:
                    raise NotImplementedError(f"'{k}': a torch.bool tensor {list(grid)} at coarse resolution (H / 8 x W / 8)")
            if self.coarse_full:
                raise NotImplementedError("padding masks with coarse.attention 'full': the published FullAttention fills a padded query row "
                                          "with -inf, its softmax is NaN and the NaN reaches every row one layer later")
        ext_c, ext_f = bool(kwargs.get("extract_coarse_feature", False)), bool(kwargs.get("extract_fine_feature", False))
        has_s = "scale0" in data
        if has_s != ("scale1" in data):
            raise NotImplementedError("'scale0' and 'scale1' come together")
        if has_s:
            for k, rows in (("scale0", (V,)), ("scale1", (V, 1) if V1 == 1 else (V,))):
                t = data[k]
                if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != 2 or t.shape[0] not in rows:
                    raise NotImplementedError(f"'{k}': a float32 tensor [{V}, 2] ([1, 2] for scale1 when image1 has batch 1)")
        fine_only = "mkpts0_c" in data
        if fine_only != ("mkpts1_c" in data):
            raise NotImplementedError("'mkpts0_c' and 'mkpts1_c' come together")
        if fine_only:
            k0, k1 = data["mkpts0_c"], data["mkpts1_c"]
            for t in (k0, k1):
                if not isinstance(t, torch.Tensor) or t.dtype not in (torch.float32, torch.float64) or t.dim() != 2 or t.shape[1] != 2:
                    raise NotImplementedError("provided coarse matches: float32 / float64 tensors [K, 2]")
            if k0.shape[0] != k1.shape[0]:
                raise NotImplementedError("'mkpts0_c' and 'mkpts1_c' must hold the same number of matches")
            if V != 1 or V1 != 1:
                raise NotImplementedError("provided coarse matches: one pair per call (the reference's b_ids are all 0)")
            if self.fine_context:
                raise NotImplementedError(FINE_ONLY_WITH_CONTEXT)
        if ext_c or ext_f:
            if V != 1 or V1 != 1:
                raise NotImplementedError("feature extraction: one pair per call (the reference squeezes scale0 to [2])")
            if ext_c and self.feature_hook is not None:
                raise NotImplementedError("extract_coarse_feature with a feature_hook: the hook's coarse rows carry the positional "
                                          "encoding, the reference samples the map before it")
            if not has_s:
                raise KeyError("scale0")
        tensors = [data["image0"], data["image1"]] + [data[k] for k in ("scale0", "scale1", "mkpts0_c", "mkpts1_c", "mask0", "mask1") if k in data]
        if not all(t.is_cuda for t in tensors):
            raise hip.HipLibraryError("LoFTR_for_OnePose_Plus runs on the HIP device only (no CPU fallback)")
        return fine_only, has_s, ext_c, ext_f

    @torch.no_grad()
    def forward(self, data, **kwargs):
        if self.training:
            raise NotImplementedError("inference only")
        # conf_matrix = "lazy" / "eager": this call's form (default: the config's); budget_bytes: what the eager re-run of a lazy call
        # that met an exact tie may allocate per sub-batch (None: all pairs at once)
        lazy = self._conf_form(kwargs.get("conf_matrix", self.conf_matrix_mode), "conf_matrix") == "lazy"
        budget = kwargs.get("budget_bytes")
        fine_only, has_s, ext_c, ext_f = self._check_inputs(data, kwargs)
        img0, img1 = data["image0"], data["image1"]
        V = img0.size(0)
        if img1.size(0) not in (1, V):
            raise ValueError(f"image1: batch {img1.size(0)} against image0's {V} (expected 1 -- one query for every pair -- or {V})")
        hip.load()
        data.update({"bs": V, "hw0_i": img0.shape[2:], "hw1_i": img1.shape[2:]})
        Wb = self._blocks(img0.device)
        debug = kwargs.get("_debug")
        fc0, fc1, ff0, ff1, fm0, fm1, hw0_c, hw1_c, hw0_f, hw1_f = self._features(Wb, data, img0, img1, debug)
        scale = img0.shape[2] / hw0_c[0]
        s0, s1 = (data["scale0"].contiguous(), data["scale1"].contiguous()) if has_s else (None, None)
        x0 = x1 = None
        if fine_only:
            mk0c, mk1c = data["mkpts0_c"], data["mkpts1_c"]
            b_ids, i_ids, j_ids = self._provided_matches(img0.device, mk0c, mk1c, img0.shape[2:], img1.shape[2:], hw0_c, hw1_c, scale, s0, s1)
            data.update({"m_bids": b_ids, "b_ids": b_ids, "i_ids": i_ids, "j_ids": j_ids, "mconf": torch.ones_like(b_ids)})
        else:
            masks = (data["mask0"], data["mask1"]) if "mask0" in data else None
            x0, x1, conf, b_ids, i_ids, j_ids, m_bids, gt_mask, mconf, mk0c, mk1c = self._coarse(Wb, fc0, fc1, hw0_c, hw1_c, scale, s0, s1, masks,
                                                                                                 lazy, budget)
            data.update({"conf_matrix": conf, "b_ids": b_ids, "i_ids": i_ids, "j_ids": j_ids, "m_bids": m_bids, "gt_mask": gt_mask,
                         "mconf": mconf, "mkpts0_c": mk0c, "mkpts1_c": mk1c})
        if self.enable_fine_matching:
            self._fine(Wb, data, ff0, ff1, b_ids, i_ids, j_ids, mk0c, mk1c, b_ids.shape[0], hw0_c, hw0_f, hw1_c, hw1_f, img0.shape[2], s1,
                       scaled=has_s or fine_only, debug=debug, x0=x0, x1=x1)
        else:
            data.update({"mkpts0_f": mk0c, "mkpts1_f": mk1c})
        if debug and x0 is not None:
            data["_feat_c0"], data["_feat_c1"] = x0, x1
        if ext_c or ext_f:
            self._extract(data, ext_c, ext_f, fm0, fm1, ff0, ff1, hw0_c, hw1_c, hw0_f, hw1_f, s0, s1)

    def _features(self, Wb, data, img0, img1, debug=False):
        """backbone (both images in one batch when their sizes agree) and the ``feature_hook`` -> coarse rows with the positional encoding
        ``fc0, fc1``, fine maps ``ff0, ff1``, coarse maps before the encoding ``fm0, fm1``, and the grids ``hw0_c, hw1_c, hw0_f, hw1_f``;
        writes the grids into ``data`` (``hw*_c``, ``hw*_f``) and, with ``debug``, the maps as the backbone left them, both ahead of the hook"""
        V, dev = img0.size(0), img0.device
        bbk = HipBackbone("bf16x3")

        def features(img):
            H, W = img.shape[2:]
            fc, ff, fm = bbk.forward(Wb["backbone"], img, self._pe_table(H // 8, W // 8, dev), return_coarse_map=True)
            return fc, ff, fm, (H // 8, W // 8), (H // 2, W // 2)
        if img0.shape[2:] == img1.shape[2:]:           # (a batch-1 query against V views: its features are computed once)
            fc, ff, fm, hw0_c, hw0_f = features(torch.cat([img0, img1], 0))
            fc0, fc1, ff0, ff1, fm0, fm1 = fc[:V], fc[V:], ff[:V], ff[V:], fm[:V], fm[V:]
            hw1_c, hw1_f = hw0_c, hw0_f
        else:
            fc0, ff0, fm0, hw0_c, hw0_f = features(img0)
            fc1, ff1, fm1, hw1_c, hw1_f = features(img1)
        data.update({"hw0_c": torch.Size(hw0_c), "hw1_c": torch.Size(hw1_c), "hw0_f": torch.Size(hw0_f), "hw1_f": torch.Size(hw1_f)})
        if debug:                                      # the backbone's maps before the positional encoding / the hook
            data.update({"_bb_c0": fm0, "_bb_c1": fm1, "_bb_f0": ff0, "_bb_f1": ff1, "_enc_c0": fc0, "_enc_c1": fc1})
        if self.feature_hook is not None:
            # one pair: the fine maps without the batch axis (the hook's form since round 3); a batch: everything with it
            if V == 1:
                fc0, f0h, fc1, f1h = self.feature_hook(fc0, ff0[0], fc1, ff1[0])
            else:
                fc0, f0h, fc1, f1h = self.feature_hook(fc0, ff0, fc1, ff1)
            ff0, ff1 = (f0h[None] if f0h.dim() == 2 else f0h), (f1h[None] if f1h.dim() == 2 else f1h)
            if fc0.shape[0] != V or fc1.shape[0] not in (1, V) or ff0.shape[0] != V or ff1.shape[0] != fc1.shape[0]:
                raise ValueError("feature_hook: batch sizes of the returned features do not match the call")
        return fc0, fc1, ff0, ff1, fm0, fm1, hw0_c, hw1_c, hw0_f, hw1_f

    def _provided_matches(self, dev, mk0c, mk1c, hw0_i, hw1_i, hw0_c, hw1_c, scale, s0, s1):
        """the fine-only branch (loftr.py:79-115): the caller's coarse keypoints clipped IN PLACE and rounded to cells; no coarse
        transformer, no matching -> ``b_ids`` (zeros), ``i_ids``, ``j_ids``"""
        K = mk0c.shape[0]
        b_ids = torch.zeros(K, dtype=torch.int64, device=dev)
        i_ids, j_ids = torch.empty(K, dtype=torch.int64, device=dev), torch.empty(K, dtype=torch.int64, device=dev)
        bad = torch.empty(1, dtype=torch.int32, device=dev)
        a0, a1 = mk0c.contiguous(), mk1c.contiguous()
        hip.launch("ophip_loftr_coarse_ids", dict(
            mkpts0=a0, mk0_double=a0.dtype == torch.float64, mkpts1=a1, mk1_double=a1.dtype == torch.float64, K=K, h0i=hw0_i[0], w0i=hw0_i[1],
            h1i=hw1_i[0], w1i=hw1_i[1], h0c=hw0_c[0], w0c=hw0_c[1], h1c=hw1_c[0], w1c=hw1_c[1], coarse_scale=scale, scale0=s0, scale1=s1,
            i_ids=i_ids, j_ids=j_ids, bad_count=bad))
        for a, t in ((a0, mk0c), (a1, mk1c)):
            if a.data_ptr() != t.data_ptr():
                t.copy_(a)
        nbad = int(bad.item()) if self.enable_fine_matching else 0      # only the fine stage indexes the maps with the ids
        if nbad:
            raise IndexError(f"{nbad} provided coarse keypoint(s) round to a cell outside the coarse grid")
        return b_ids, i_ids, j_ids

    def _coarse(self, Wb, fc0, fc1, hw0_c, hw1_c, scale, s0, s1, masks, lazy=False, budget=None):
        """coarse transformer and coarse matching between the two grids; ``masks``: None or ``(mask0, mask1)`` as the caller gave them
        -> final rows ``x0, x1``, ``conf_matrix`` and the K matches ``b_ids, i_ids, j_ids, m_bids, gt_mask, mconf, mkpts0_c, mkpts1_c``.
        ``lazy``: no ``[V, L0, L1]`` tensor is allocated, ``conf_matrix`` is a :class:`LazyConfMatrix`; an exact row tie that the
        selection cannot resolve without the stored row (``count[1]``) runs the matching again eagerly on the same rows, in sub-batches of
        pairs whose :meth:`coarse_batch_bytes` fits ``budget`` (None: all at once)"""
        V, dev = fc0.shape[0], fc0.device
        L0, L1 = hw0_c[0] * hw0_c[1], hw1_c[0] * hw1_c[1]
        # ---- coarse transformer.  linear: self = one two-stream launch, cross = two one-stream launches (sequential semantics);
        #      full: one one-stream launch per image and layer, the shared query read with batch stride 0 -----------------------
        if masks is not None:                          # flattened, the query's repeated for every pair (read only: never written)
            m1 = masks[1].reshape(-1, L1)
            masks = (masks[0].reshape(V, L0).contiguous(), (m1.expand(V, -1) if m1.shape[0] != V else m1).contiguous())
        if self.coarse_full:
            x0, x1 = self._coarse_full(Wb["coarse"], fc0.contiguous(), fc1.contiguous(), V, L0, L1)
        else:
            x0, x1 = self._coarse_linear(Wb["coarse"], fc0, fc1, fc1.shape[0] == 1 and V > 1, V, L0, L1, masks)

        # ---- coarse matching between the two grids -------------------------------------------------------------------------
        def match(y0, y1, mk, want_conf=True):
            return self._match(Wb["bin_score"], y0, y1, mk, hw0_c, hw1_c, scale, want_conf)
        raw = match(x0, x1, masks, not lazy)
        # the detector reads the matches on the host right after: one sync here (the count and the lazy form's tie flag in one copy)
        K, tie = raw.count[:2].tolist()
        if lazy and tie:
            self.lazy_reruns += 1
            n = V
            if budget is not None:                         # the largest sub-batch within the budget, one pair at the least
                while n > 1 and self.coarse_batch_bytes(n, hw0_c, hw1_c, False) > budget:
                    n -= 1
            parts = []
            for p in range(0, V, n):                       # ascending (b, i) inside a sub-batch: pair order is the full call's order
                sub = match(x0[p:p + n], x1[p:p + n], None if masks is None else (masks[0][p:p + n], masks[1][p:p + n]))
                parts.append(self._lists(sub, int(sub.count[0].item()), p))
            lists = tuple(torch.cat([q[k] for q in parts], 0) for k in range(8))
        else:
            lists = self._lists(raw, K, 0)
        conf = raw.conf
        if lazy:
            conf = LazyConfMatrix(lambda y0, y1, mk: match(y0, y1, mk).conf, x0, x1, masks, torch.cuda.current_stream(dev))
        b_ids, i_ids, j_ids, m_bids, gt_mask, mconf, mk0c, mk1c = lists
        if s0 is not None:                                 # get_coarse_match: cell * (scale * scale0[b_ids]); scale = 8 is a power of two
            mk0c = mk0c * s0[b_ids]
            mk1c = mk1c * (s1[b_ids] if s1.shape[0] > 1 else s1)
        return x0, x1, conf, b_ids, i_ids, j_ids, m_bids, gt_mask, mconf, mk0c, mk1c

    def _match(self, bin_score, x0, x1, masks, hw0_c, hw1_c, scale, want_conf):
        """one coarse-matching call on the final rows ``x0 [V, L0, 256]``, ``x1 [V, L1, 256]`` (``masks``: None or the flattened pair) ->
        the entry point's output buffers of capacity ``V * L0`` and ``count`` (int32 ``[4]`` on the device: the number of matches and,
        without ``want_conf``, the tie flag); ``conf`` is ``None`` without ``want_conf`` (dual softmax only: the lazy form)"""
        V, L0, dev = x0.shape[0], x0.shape[1], x0.device
        mc = self.config["match_coarse"]
        ii = torch.arange(L0, device=dev)
        pts0 = torch.stack([(ii % hw0_c[1]).float() * scale, (ii // hw0_c[1]).float() * scale, torch.zeros(L0, device=dev)], 1)[None].contiguous()
        lists = MatchLists.empty(V * L0, dev, conf_shape=(V, L0, x1.shape[1]) if want_conf else None)
        form = (dict(sinkhorn=(bin_score, int(mc["skh_iters"]), 1 if mc["skh_prefilter"] else 0)) if self.sinkhorn
                else dict(temperature=mc["dsmax_temperature"]))
        coarse_match_2d(x0, x1, pts0, w0c=hw0_c[1], w1c=hw1_c[1], thr=mc["thr"], border_rm=mc["border_rm"], scale=scale, lists=lists,
                        conf=lists.conf, masks=masks, **form)
        return lists

    @staticmethod
    def _lists(raw, K, first_pair):
        """the K matches of one :meth:`_match` call, ``b_ids`` counted from ``first_pair`` -> ``b_ids, i_ids, j_ids, m_bids, gt_mask,
        mconf, mkpts0_c, mkpts1_c`` (the keypoints before the image scales)"""
        b_ids, i_ids, j_ids, m_bids, gt_mask, mconf, mk0, mk1c = raw.trim(K)
        if first_pair:
            b_ids, m_bids = b_ids + first_pair, m_bids + first_pair
        return b_ids, i_ids, j_ids, m_bids, gt_mask, mconf, mk0[:, :2].contiguous(), mk1c.contiguous()

    def _fine(self, Wb, data, ff0, ff1, b_ids, i_ids, j_ids, mk0c, mk1c, K, hw0_c, hw0_f, hw1_c, hw1_f, h0i, s1, scaled, debug,
              b_ids1=None, scale_ids=None, x0=None, x1=None):
        """fine stage (windows on both images, two-stream fine transformer, correlation + soft-argmax) on the matches' cells.
        ``b_ids1`` / ``scale_ids`` (``sfm_fine``: every row names its own two images): the batch index into ``ff1`` and the row of ``s1``
        when they are not ``b_ids``.  ``x0 [V, L0, 256]``, ``x1 [V, L1, 256]``: the coarse transformer's final rows, which a matcher with
        ``fine_concat_coarse_feat`` merges into the windows (``fine_context.merge``, in place) ahead of the fine transformer"""
        b_ids1 = b_ids if b_ids1 is None else b_ids1
        scale_ids = b_ids if scale_ids is None else scale_ids
        dev = ff0.device
        Wf = int(self.config["fine_window_size"])
        WW = Wf * Wf
        if K == 0:
            data.update({"expec_f": torch.empty(0, 3, device=dev), "mkpts0_f": mk0c, "mkpts1_f": mk1c})
            return
        stride = hw0_f[0] // hw0_c[0]
        f0, f1 = torch.empty(K, WW, 128, device=dev), torch.empty(K, WW, 128, device=dev)
        ff0c, ff1c = ff0.contiguous(), ff1.contiguous()          # [V or 1][hf * wf][128] channels-last
        hip.launch("ophip_fine2_gather_b", dict(feat_cl=ff0c, feat_bstride=ff0c.stride(0) if ff0c.shape[0] > 1 else 0, b_ids=b_ids, hf=hw0_f[0],
                                                wf=hw0_f[1], cell_ids=i_ids, K=K, wc=hw0_c[1], stride=stride, W=Wf, out=f0))
        hip.launch("ophip_fine2_gather_b", dict(feat_cl=ff1c, feat_bstride=ff1c.stride(0) if ff1c.shape[0] > 1 else 0, b_ids=b_ids1, hf=hw1_f[0],
                                                wf=hw1_f[1], cell_ids=j_ids, K=K, wc=hw1_c[1], stride=hw1_f[0] // hw1_c[0], W=Wf, out=f1))
        if self.fine_context:
            if x0 is None or x1 is None:
                raise NotImplementedError(FINE_ONLY_WITH_CONTEXT)
            fine_context.merge(f0, f1, x0, x1, b_ids, i_ids, j_ids, Wf, Wb["context"])
            if debug:                                  # the windows the fine transformer reads (its layers write new tensors)
                data["_fine_in0"], data["_fine_in1"] = f0, f1
        T = K * WW

        def attention(q, k, v, msg):
            named = dict(q=q, k=k, v=v, K=K, L=WW, S=WW, msg=msg)
            if self.fine_full:
                hip.launch("ophip_fine2_full_attention", named)
            else:
                hip.launch("ophip_fine2_attention", named)

        def fine_layer(x, src, w):
            return rows_encoder_layer(x, T, src, T, w, attention)
        for w, name in zip(Wb["fine"], self.loftr_fine.layer_names):
            if name == "self":
                f0, f1 = fine_layer(f0, f0, w), fine_layer(f1, f1, w)
            else:
                f0 = fine_layer(f0, f1, w)
                f1 = fine_layer(f1, f0, w)
        expec = torch.empty(K, 3, device=dev)
        if scaled:
            # FineMatching with 'scale0' in data: mkpts1_c + coords * (W // 2) * (scale * scale1[b_ids]), in mkpts1_c's dtype.  The
            # fine-only branch without scales uses the plain scale: the same arithmetic with unit scales
            s1 = s1 if s1 is not None else torch.ones(1, 2, device=dev)
            mk1c_ = mk1c.contiguous()
            mk1f = torch.empty(K, 2, dtype=mk1c.dtype, device=dev)
            hip.launch("ophip_fine2_match_scaled", dict(f0=f0, f1=f1, mkpts1_c=mk1c_, mk_double=mk1c.dtype == torch.float64, b_ids=scale_ids,
                                                        scale1=s1, scale1_bstride=2 if s1.shape[0] > 1 else 0, K=K, W=Wf, scale=h0i / hw0_f[0],
                                                        expec_f=expec, mkpts1_f=mk1f))
        else:
            mk1f = torch.empty(K, 2, device=dev)
            hip.launch("ophip_fine2_match", dict(f0=f0, f1=f1, mkpts1_c=mk1c, K=K, W=Wf, scale=(Wf // 2) * (h0i / hw0_f[0]), expec_f=expec,
                                                 mkpts1_f=mk1f))
        data.update({"expec_f": expec, "mkpts0_f": mk0c, "mkpts1_f": mk1f})
        if debug:
            data["_fine_f0"], data["_fine_f1"] = f0, f1

    def _extract(self, data, ext_c, ext_f, fm0, fm1, ff0, ff1, hw0_c, hw1_c, hw0_f, hw1_f, s0, s1):
        """loftr.py:131-167: backbone features at mkpts*_f -- the coarse map before the positional encoding (nearest) and the fine map
        (bilinear), keypoints normalised by scale * hw_i; one ``ophip_sample_features`` launch for all of them"""
        dev = fm0.device
        jobs, outs = [], {}
        hw0_i, hw1_i = data["hw0_i"], data["hw1_i"]
        k0, k1 = data["mkpts0_f"].contiguous(), data["mkpts1_f"].contiguous()
        todo = []
        if ext_c:
            todo += [("feat_coarse_b_0", fm0, hw0_c, 256, k0, s0, hw0_i, 1), ("feat_coarse_b_1", fm1, hw1_c, 256, k1, s1, hw1_i, 1)]
        if ext_f:
            todo += [("feat_ext0", ff0, hw0_f, 128, k0, s0, hw0_i, 0), ("feat_ext1", ff1, hw1_f, 128, k1, s1, hw1_i, 0)]
        for name, fmap, hw, C, kp, sc, hw_i, nearest in todo:
            fmap = fmap.contiguous()
            if tuple(fmap.shape[-2:]) != (hw[0] * hw[1], C):
                raise ValueError(f"{name}: map of shape {tuple(fmap.shape)}, expected [{hw[0] * hw[1]}, {C}]")
            out = torch.empty(kp.shape[0], C, device=dev)
            outs[name] = (out, fmap, kp, sc)            # keep the operands alive until the launch is enqueued
            jobs.append(hip.SampleJob(fmap.data_ptr(), kp.data_ptr(), sc.data_ptr(), out.data_ptr(), hw[0], hw[1], C, kp.shape[0],
                                      hw_i[0], hw_i[1], int(kp.dtype == torch.float64), nearest))
        arr = (hip.SampleJob * len(jobs))(*jobs)
        hip.launch("ophip_sample_features", dict(jobs=arr, n_jobs=len(jobs)))
        data.update({name: o[0] for name, o in outs.items()})


def build_2D_match_model(args: dict) -> LoFTR_for_OnePose_Plus:
    """``local_feature_2D_detector.py:24-37``: LoFTR with the default config, checkpoint loaded strictly (``weights_only=True``:
    nothing from the file is executed), ``eval()``.  The reference also seeds the global generators (``pl.seed_everything``): inference
    draws no random numbers, so there is nothing to seed here.  ``args["config"]`` (optional, this build's): another config, e.g. the
    published LoFTR one (``fine_concat_coarse_feat`` True, window 5) for the public checkpoints."""
    if args["method"] != "LoFTR":
        raise NotImplementedError
    matcher = LoFTR_for_OnePose_Plus(config=copy.deepcopy(args.get("config") or default_cfg))
    state_dict = torch.load(args["weight_path"], map_location="cpu", weights_only=True)["state_dict"]
    return load_matcher_checkpoint(matcher, state_dict)
