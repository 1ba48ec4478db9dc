"""Drop-in ``OnePosePlus_model`` whose hot path runs on hand-written gfx950 kernels.

Mirrors the reference interface (``src/models/OnePosePlus/OnePosePlusModel.py:24-203``):

* ``OnePosePlus_model(config, profiler=None, debug=False)`` with the ``model.OnePosePlus``
  config block; unsupported values raise ``NotImplementedError`` / ``ValueError`` as the
  reference does.
* the same ``state_dict`` key layout (195 tensors), so ``build_model`` /
  ``load_state_dict(strict=True)`` of a reference checkpoint works
  (``src/inference/inference_OnePosePlus.py:30-40``).
* ``model(data) -> None`` mutating ``data`` with exactly the keys, dtypes and shapes the
  reference writes.

The ``nn`` sub-modules below only *hold parameters* under the reference's names; the
arithmetic of rows a1-a11 is done by ``libonepose_hip.so`` through its C ABI
(``include/onepose_hip.h``).  The ResNet-FPN backbone runs on the
hand-written convolution kernels as well (``backbone_hip.py``; ``config["hip_backbone"] = False``
or the exact-f32 mode keep it on PyTorch-ROCm / MIOpen).  There is no CPU fallback: calling the
model without the HIP library or with CPU tensors raises.
"""
from __future__ import annotations

import contextlib
import ctypes
import os
import weakref
from collections import namedtuple

import torch
import torch.nn as nn

from . import hip, host_math, layercall, ops, packing, supervision, train_forward
from .backbone import build_backbone
from .backbone_hip import HipBackbone, pack_backbone
from .config import encoder_layer_names, validate_config
from .hip import bstride
from .lazy_conf import LazyConfMatrixBase
from .matchcall import MatchLists, coarse_match, fine_refine
from .params import EncoderParams, load_matcher_checkpoint
from .rows import rows_encoder_layer


class _KeypointEncoderParams(nn.Module):
    """``KeypointEncoding_linear`` parameter holder: Linear at indices 0, 3, 6, 9
    (position_encoding.py:62-79; the norm / ReLU slots carry no parameters)."""

    def __init__(self, inp_dim, feature_dim, layers):
        super().__init__()
        chans = [inp_dim] + list(layers) + [feature_dim]
        mods = []
        for i in range(1, len(chans)):
            mods.append(nn.Linear(chans[i - 1], chans[i], bias=True))
            if i < len(chans) - 1:
                mods += [nn.Identity(), nn.Identity()]
        self.encoder = nn.Sequential(*mods)
        nn.init.constant_(self.encoder[-1].bias, 0.0)


_stream_objs = {}


def _current_stream(dev):
    """``torch.cuda.current_stream(dev)`` without its ~8 us of Python (lazy-init and device-index helpers) on the per-frame path: the raw
    handle of the current stream is one C call, the Stream object that wraps it is looked up by (device, handle)."""
    idx = dev.index
    if idx is None:
        return torch.cuda.current_stream(dev)
    raw = torch._C._cuda_getCurrentRawStream(idx)
    st = _stream_objs.get((idx, raw))
    if st is None:
        st = torch.cuda.current_stream(dev)
        if len(_stream_objs) >= 64:
            _stream_objs.clear()
        _stream_objs[(idx, raw)] = st
    return st


_NSPLIT = {"f32": 0, "bf16": 1, "bf16x3": 3}          # hip_precision -> the operand split the matching and fine kernels take


def _side_stream(table, key, dev, priority=0, with_event=False):
    """The side stream ``table`` keeps for ``key``, created on first use.  The tables are keyed on the raw handle of a compute stream, so
    each holds 16 entries at most and drops its oldest instead of growing for ever.  ``with_event``: the entry is ``[stream, last event]``
    (the fine streams) and is returned whole."""
    ent = table.get(key)
    if ent is None:
        if len(table) >= 16:
            table.pop(next(iter(table)))
        st = torch.cuda.Stream(device=dev, priority=priority)
        ent = table[key] = [st, None] if with_event else st
    return ent


def _dense(t):
    return t if (t.dtype == torch.float32 and t.is_contiguous()) else t.float().contiguous()


def _per_frame(t):        # [B or 1, ...] dense per frame, without materialising an expand()
    if t.stride(0) == 0 and t.shape[0] > 1:
        t = t[:1]
    return _dense(t)


# one ``enqueue_features`` call's checked inputs: sizes, device, the object block dense per frame (batch 1 when the frames share it), the
# query images' optional padding mask [B, M] uint8 and scale [B, 2], the packed weights
FrameInputs = namedtuple("FrameInputs", "B N M hc wc hf wf dev kpts_d desc_in_d desc_fine_d qmask qscale W")


class _NullProfiler:
    _scope = contextlib.nullcontext()

    def record_function(self, name):
        return self._scope


class OnePosePlus_model(nn.Module):
    def __init__(self, config, profiler=None, debug=False):
        super().__init__()
        validate_config(config)
        self.config = config
        self.profiler = profiler or _NullProfiler()
        self.debug = debug
        cc, cf = config["loftr_coarse"], config["loftr_fine"]
        if cc["d_model"] != 256 or cc["nhead"] != 8:
            raise NotImplementedError("HIP coarse encoder is specialised for d_model=256, nhead=8")
        if cf["d_model"] != 128 or cf["nhead"] != 8 or cf["window_size"] != 5:
            raise NotImplementedError("HIP fine stage is specialised for d_model=128, nhead=8, window 5")

        self.backbone = build_backbone(config["loftr_backbone"])
        self.kpt_3d_pos_encoding = None
        if config["keypoints_encoding"]["enable"]:
            ke = config["keypoints_encoding"]
            if ke["descriptor_dim"] != 256 or list(ke["keypoints_encoder"]) != [32, 64, 128]:
                raise NotImplementedError("HIP keypoint encoder is specialised for 3->32->64->128->256")
            self.kpt_3d_pos_encoding = _KeypointEncoderParams(3, ke["descriptor_dim"], ke["keypoints_encoder"])
        self.loftr_coarse = EncoderParams(encoder_layer_names(cc), cc["d_model"], cc["nhead"])
        self.loftr_fine = EncoderParams(encoder_layer_names(cf), cf["d_model"], cf["nhead"])
        self._pe_enable = bool(config["positional_encoding"]["enable"])
        self._pe_shape = tuple(config["positional_encoding"]["pos_emb_shape"])
        # matrix arithmetic of the HIP kernels:
        #   "bf16x3" (default) split-bf16 MFMA, 3 x v_mfma_f32_32x32x16_bf16 per product, f32 accumulate: ~f32-grade
        #   "f32"    exact-f32 MFMA (v_mfma_f32_32x32x2_f32, bit-for-bit an fmaf chain), 1/16 of the bf16 rate
        #   "bf16"   plain bf16 operands: fastest, ~1e-2 relative on activations
        self.precision = str(config.get("hip_precision", os.environ.get("OPHIP_PRECISION", "bf16x3")))
        if self.precision not in ("f32", "bf16x3", "bf16"):
            raise ValueError(f"hip_precision {self.precision!r}: expected 'f32', 'bf16x3' or 'bf16'")
        # loftr_coarse.attention = "full" (transformer.py:29-38): softmax attention in the coarse encoder, on the split-bf16 flash-attention
        # kernel of csrc/encoder_full.hip; it runs the stage-by-stage path in the default arithmetic mode only
        self.coarse_full = cc["attention"] == "full"
        if self.coarse_full and self.precision != "bf16x3":
            raise NotImplementedError(f"loftr_coarse.attention = 'full' runs with hip_precision 'bf16x3' only (got {self.precision!r})")
        # loftr_fine.attention = "full": the fine stage composed over all matches from row kernels (csrc/fine_full.hip, ophip_rows_linear_x3),
        # split-bf16 linear layers; its own arithmetic, so neither the plain-bf16 mode nor the plain-bf16 fine stage applies
        self.fine_full = cf["attention"] == "full"
        if self.fine_full and self.precision != "bf16x3":
            raise NotImplementedError(f"loftr_fine.attention = 'full' runs with hip_precision 'bf16x3' only (got {self.precision!r})")
        if self.fine_full and config.get("hip_fine_precision") is not None and str(config["hip_fine_precision"]) != "bf16x3":
            raise NotImplementedError("loftr_fine.attention = 'full' runs with hip_fine_precision 'bf16x3' only")
        # the FINE stage's arithmetic when the path runs in "bf16x3": "bf16x3" (default: every keypoint within 1e-4 relative of the reference's)
        # or "bf16" -- plain bf16 operands, a third of the stage's matrix work: match indices unchanged (the fine stage only moves a match's
        # sub-pixel offset), keypoints within 0.05 px, pose within 1e-5 of the default's (tests/test_gpu_parity.py::test_fine_stage_in_plain_bf16...).
        # The library reads the switch from the environment on every fine-stage launch, so the key is PROCESS-WIDE: giving it sets
        # OPHIP_FINE_PRECISION for every model of the process; leaving it out keeps whatever the environment says (default "bf16x3").
        fp = config.get("hip_fine_precision")
        if fp is not None:
            if str(fp) not in ("bf16x3", "bf16"):
                raise ValueError(f"hip_fine_precision {fp!r}: expected 'bf16x3' or 'bf16'")
            os.environ["OPHIP_FINE_PRECISION"] = str(fp)
        # backbone on the HIP convolution kernels (bf16 pipe modes only; exact-f32 mode keeps MIOpen's fp32 convolutions)
        self.hip_backbone = bool(config.get("hip_backbone", True)) and self.precision != "f32"
        self.lazy_reruns = 0          # lazy conf_matrix: frames re-run eagerly because of an exact row tie (PendingFrame.finish)
        self._packed = None          # (key, dict of device weight blocks)
        self._packed_bb = None       # (key, backbone conv blocks)
        # fine stage (+ result read-back) on a second HIP stream: frame t's refinement then overlaps frame t + 1's input
        # kernels (PE add, transposes, keypoint encoding, backbone); frame t + 1's encoder waits for it, so the two
        # MFMA-heavy stages never share the chip
        self.overlap_fine = bool(config.get("hip_overlap_fine", True))
        self._fine_streams = {}      # (device, compute stream) -> (fine stream, last fine-done event)
        self._prep_streams = {}      # (device, compute stream) -> input-kernel stream (enqueue_features(inputs_ready=True))
        self._pe_cache = {}          # (h, w, device) -> [M, C] device table
        # per-object cache of the frame-invariant keypoint encoding (rows a2 + a3); off by default so that a forward always does
        # all of its work unless the caller opts in (bench.py reports both)
        self.cache_object = bool(config.get("hip_cache_object", False))
        self._obj_cache = None
        # conf_matrix: "eager" (default) stores the N x M matrix every frame like the reference; "lazy" never stores it (the
        # inference callers read only the match lists): ``data["conf_matrix"]`` is then a :class:`LazyConfMatrix` that materialises on
        # first use.  Match indices and confidences are bit-identical in both forms.
        self.conf_matrix_mode = str(config.get("hip_conf_matrix", "eager"))
        if self.conf_matrix_mode not in ("eager", "lazy"):
            raise ValueError(f"hip_conf_matrix {self.conf_matrix_mode!r}: expected 'eager' or 'lazy'")
        if self.conf_matrix_mode == "lazy" and self.precision == "f32":
            raise ValueError("hip_conf_matrix = 'lazy' needs a bf16 arithmetic mode (the exact-f32 mode always materialises conf_matrix)")
        # the default path as ONE C call per frame (csrc/frame.hip: same kernels, same streams, one device block per frame) instead of
        # ~27 ctypes calls + ~20 allocations + ~10 stream / event operations from Python: 0.39 -> ~0.1 ms of host time per frame
        self.frame_call = bool(config.get("hip_frame_call", os.environ.get("OPHIP_FRAME_CALL", "1") != "0"))
        self._frame_plans = {}
        # ids this model holds in ops._frame_plans (whose entries keep the packed weight blocks alive): released when the model is collected
        self._plan_ids = set()
        weakref.finalize(self, ops.drop_frame_plans, self._plan_ids)
        self._frame_call_pending = set()     # compute streams whose last frame went through the C entry point
        # the training-mode forward (off: a training-mode call raises): the eval forward stage by stage on the current
        # stream with conf_matrix stored, and between its coarse and fine stages the reference's GT padding (train_forward.pad_matches).
        # Its draws are (hip_train_seed, train_calls): the model counts its training calls; reseed() sets both.
        self.train_forward = bool(config.get("hip_train_forward", False))
        self.train_seed = int(config.get("hip_train_seed", 0))
        self.train_calls = 0
        # the training-mode forward also leaves the four feature tensors the loss backward starts from (loss_backward.backward; DESIGN.md
        # section 6u) in ``data``: feat_c0 / feat_c1 (the coarse encoder's outputs) and feat_f0 / feat_f1 (the fine encoder's, at the
        # lists' capacity).  Off: no key of ``data`` changes and no buffer is allocated.
        self.keep_features = bool(config.get("hip_keep_features", False))
        # the training-mode forward also keeps every coarse layer's inputs for the coarse transformer's backward (encoder_backward.coarse_backward;
        # DESIGN.md section 6v): each layer then writes fresh buffers instead of the ping-pong pair, and ``data["layer_inputs_c"]`` is the list
        # of ``(x3d, x2d)`` per layer.  Off: no key of ``data`` changes, no buffer is allocated, the same bytes come out.
        self.keep_layer_inputs = bool(config.get("hip_keep_layer_inputs", False))

        pretrained = config["loftr_backbone"]["pretrained"]
        if pretrained is not None:
            # OnePosePlusModel.py:78-93: take the `backbone.*` entries of a LoFTR checkpoint
            ckpt = torch.load(pretrained, map_location="cpu", weights_only=True)["state_dict"]
            sub = {k[k.find("backbone") + len("backbone") + 1:]: v for k, v in ckpt.items() if "backbone" in k}
            self.backbone.load_state_dict(sub)
            if config["loftr_backbone"]["pretrained_fix"]:
                for p in self.backbone.parameters():
                    p.requires_grad = False

    # ------------------------------------------------------------------------------------------
    # device-side weight blocks (re-packed when parameters change or move)
    # ------------------------------------------------------------------------------------------
    _PARAM_REWALK = 64          # frames between two full walks of the module tree in _weights() (a backstop: see _matcher_params)

    def _matcher_params(self):
        """The parameters whose packed copies the kernels read, as a list that is NOT rebuilt on every frame: walking the module tree
        (``named_parameters``: 145 tensors below ~40 modules) cost ~100 us of a 690 us frame period -- a third of the host time of an
        enqueue -- for a question whose answer changes when a user edits the model.  The list is rebuilt every ``_PARAM_REWALK`` frames,
        whenever ``_apply`` (``.to`` / ``.cuda`` / ``.float``) or ``load_state_dict`` ran, and whenever the tree itself changed: beside the
        list the cache keeps every (module, name, Parameter) and (parent, name, sub-module) edge it was built from and re-checks their
        identity on each frame (~190 dictionary look-ups, ~15 us), so a replaced Parameter (``layer.q_proj.weight = nn.Parameter(...)``,
        ``load_state_dict(assign=True)`` on a sub-module, ``parametrize``) or a replaced sub-module is seen on the very next frame; a
        parameter that is written in place or moved is caught by the (data_ptr, _version) key of ``_weights``."""
        c = self.__dict__.get("_param_cache")
        if c is not None and c[1] > 0:
            for mod, name, p in c[2]:
                if mod._parameters.get(name) is not p:
                    c = None
                    break
            else:
                for parent, name, child in c[3]:
                    if parent._modules.get(name) is not child:
                        c = None
                        break
        if c is None or c[1] <= 0:
            pedges, medges, plist = [], [], []
            stack = [(n, m) for n, m in self._modules.items() if n != "backbone" and m is not None]
            medges += [(self, n, m) for n, m in stack]
            while stack:
                _, mod = stack.pop()
                for n, p in mod._parameters.items():
                    if p is not None:
                        pedges.append((mod, n, p))
                for n, ch in mod._modules.items():
                    if ch is not None:
                        medges.append((mod, n, ch))
                        stack.append((n, ch))
            plist = [p for n, p in self.named_parameters() if not n.startswith("backbone.")]
            c = self.__dict__["_param_cache"] = [plist, self._PARAM_REWALK, pedges, medges]
        c[1] -= 1
        return c[0]

    def _apply(self, fn, *args, **kwargs):
        self.__dict__["_param_cache"] = None
        return super()._apply(fn, *args, **kwargs)

    def load_state_dict(self, *args, **kwargs):
        self.__dict__["_param_cache"] = None
        return super().load_state_dict(*args, **kwargs)

    def _weights(self, device):
        params = self._matcher_params()
        key = (str(device), self.precision, tuple([p.data_ptr() for p in params]), tuple([p._version for p in params]))
        if self._packed is not None and self._packed[0] == key:
            return self._packed[1]
        self.__dict__["_param_cache"] = None              # a change: the next frame walks the tree again
        params = self._matcher_params()
        key = (str(device), self.precision, tuple([p.data_ptr() for p in params]), tuple([p._version for p in params]))
        sd = {k: v for k, v in self.state_dict().items() if not k.startswith("backbone.")}
        n_fine = len(self.loftr_fine.layer_names)

        def coarse(pack):
            return [pack(sd, f"loftr_coarse.layers.{i}.").to(device) for i in range(len(self.loftr_coarse.layer_names))]
        blocks = {"coarse": coarse(packing.pack_coarse_layer),
                  "fine": torch.cat([packing.pack_fine_layer(sd, f"loftr_fine.layers.{i}.") for i in range(n_fine)]).to(device)}
        if self.kpt_3d_pos_encoding is not None:
            blocks["kpt"] = packing.pack_keypoint_encoder(sd).to(device)
        if self.precision == "bf16":
            blocks["coarse_bf16"] = coarse(packing.pack_coarse_layer_bf16)
        if self.precision == "bf16x3":
            blocks["coarse_x3"] = coarse(packing.pack_coarse_layer_x3w8)
        if self.fine_full:
            blocks["fine_full"] = [{n: t.to(device) for n, t in packing.pack_fine_layer_full_x3(sd, f"loftr_fine.layers.{i}.").items()} for i in range(n_fine)]
        if self.precision != "f32":
            blocks["fine_bf16"] = packing.pack_fine_layers_bf16(sd, "loftr_fine.layers.", n_fine).to(device)
        self._packed = (key, blocks)
        return blocks

    def _backbone_blocks(self, device):
        tensors = list(self.backbone.state_dict().values())
        key = (str(device),) + tuple((t.data_ptr(), t._version) for t in tensors)
        if self._packed_bb is None or self._packed_bb[0] != key:
            self._packed_bb = (key, pack_backbone(self.backbone.state_dict(), device))
        return self._packed_bb[1]

    def _pe_table(self, h, w, device):
        k = (h, w, str(device))
        if k not in self._pe_cache:
            self._pe_cache[k] = host_math.pe_table(self.config["loftr_coarse"]["d_model"], h, w, self._pe_shape).to(device)        # [M, C]
        return self._pe_cache[k]

    # ------------------------------------------------------------------------------------------
    def forward(self, data):
        """Same contract as the reference ``forward`` (OnePosePlusModel.py:95-203)."""
        self.enqueue(data).finish()

    def enqueue(self, data, host_copy=False):
        """``forward`` without the final wait: backbone + rows a1-a11 enqueued on the current stream; returns the
        :class:`PendingFrame` (see :meth:`enqueue_features`)."""
        if self.training and not self.train_forward:
            raise NotImplementedError("the HIP path implements inference; call .eval() (training padding "
                                      "of coarse_matching.py:177-217 is out of scope)")
        if "mask0" in data:
            raise NotImplementedError("data['mask0']: not implemented (the reference raises as well, coarse_matching.py:149-152)")
        data.update({"bs": data["query_image"].size(0), "q_hw_i": data["query_image"].shape[2:]})
        img = data["query_image"]
        if self.hip_backbone and not self.training:          # training: torch's BatchNorm in training mode is the reference's; the folded-BN convolutions are eval arithmetic
            feat_c, feat_f = self.backbone_features(img)
            return self.enqueue_features(data, feat_c, feat_f, host_copy=host_copy, _pe_applied=True)
        with torch.no_grad():
            feat_c, feat_f = self.backbone(img)
        return self.enqueue_features(data, feat_c, feat_f, host_copy=host_copy)

    def backbone_features(self, img):
        """Row f-1 on the HIP convolution kernels: ``[B, 1, H, W]`` image -> ``(feat_c, feat_f)`` with the reference's
        ``[B, C, h, w]`` shapes over channels-last memory; the positional encoding (row a1) is already added to ``feat_c``."""
        if not self.hip_backbone:
            raise RuntimeError("hip_backbone is disabled for this model (exact-f32 mode or config['hip_backbone'] = False)")
        if not img.is_cuda:
            raise hip.HipLibraryError("OnePosePlus_model runs on the HIP device only (no CPU fallback): move the "
                                      "model and its inputs to 'cuda'")
        B, _, H, W = img.shape
        pe = self._pe_table(H // 8, W // 8, img.device) if self._pe_enable else None
        fc, ff = HipBackbone(self.precision).forward(self._backbone_blocks(img.device), img, pe)
        return (fc.view(B, H // 8, W // 8, fc.shape[2]).permute(0, 3, 1, 2), ff.view(B, H // 2, W // 2, ff.shape[2]).permute(0, 3, 1, 2))

    def forward_features(self, data, feat_c, feat_f, image_hw=None, want_fine_debug=False):
        """The north_star path: everything after the backbone.  ``feat_c [B,256,H/8,W/8]``,
        ``feat_f [B,128,H/2,W/2]`` (any strides); fills ``data`` like :meth:`forward`."""
        self.enqueue_features(data, feat_c, feat_f, image_hw, want_fine_debug).finish()

    @torch.no_grad()
    def enqueue_features(self, data, feat_c, feat_f, image_hw=None, want_fine_debug=False, host_copy=False, _pe_applied=False,
                         inputs_ready=False, _force_eager=False):
        """Enqueue the whole path for one batch on the current stream WITHOUT synchronising and return a
        :class:`PendingFrame`; ``.finish()`` waits for that frame only (an event, not the stream) and fills ``data``.
        A pipeline enqueues frame t + 1 before finishing frame t, so the GPU never idles on the host
        (``bench.py``).  The fine stage runs on a second stream (``config["hip_overlap_fine"]``, default on): the inputs
        must stay unmodified until ``finish()``.  ``host_copy=True`` also queues the D2H of the match buffers into pinned memory, which
        ``finish()`` exposes as numpy arrays (``pending.host``) for host PnP.  ``inputs_ready=True``: the caller guarantees that
        ``feat_c``, ``feat_f`` and the object block are complete in device memory (nothing that writes them is still queued), so
        the input kernels may run on a side stream ahead of the work already queued on the current one."""
        fi = self._frame_inputs(data, feat_c, feat_f, image_hw)
        main = _current_stream(fi.dev)
        fkey = (str(fi.dev), main.cuda_stream)
        if self.training and self.train_forward:
            return self._enqueue_training(data, feat_c, feat_f, fi, main, fkey, want_fine_debug, host_copy, _pe_applied)
        lazy = self.conf_matrix_mode == "lazy" and not _force_eager
        # a lazy frame whose selection meets an exact row tie it cannot resolve without the stored row is run again with conf_matrix
        rerun = (lambda: self.enqueue_features(data, feat_c, feat_f, image_hw, want_fine_debug, host_copy, _pe_applied, False, True)) if lazy else None
        if (self.frame_call and self.precision == "bf16x3" and not self.coarse_full and not self.fine_full and self.overlap_fine and not _pe_applied and not want_fine_debug
                and not self.debug and bool(self.config["fine_matching"]["enable"])
                and (self.kpt_3d_pos_encoding is not None or fi.B == 1 or fi.desc_in_d.shape[0] == fi.B)
                and len(self.loftr_coarse.layer_names) <= 16):
            return self._enqueue_frame_call(data, feat_c, feat_f, fi, main, fkey, host_copy, inputs_ready, lazy, rerun)
        # the same frame stage by stage, every launch issued from Python
        if fkey in self._frame_call_pending:                          # order this frame's encoder behind the C path's last fine stage
            self._frame_call_pending.discard(fkey)
            hip.call("ophip_frame_order_after_fine", ctypes.c_void_p(main.cuda_stream))
        x2d, x3d, ff, ff_strides = self._input_stage(fi, feat_c, feat_f, main, fkey, _pe_applied, inputs_ready)      # a1, fine map, a2 + a3
        x3d, x2d = self._coarse_encoder_stage(fi, x3d, x2d, main, fkey)                                              # a4-a6
        if self.debug:
            data["_feat3d_c"], data["_feat2d_c"] = x3d, x2d
        cb, select = self._coarse_matching_stage(data, fi, x3d, x2d, main, lazy)                                     # a7 + a8
        pend = self._fine_stage(data, fi, cb, select, ff, ff_strides, main, fkey, want_fine_debug, host_copy)      # a9-a11
        pend._rerun = rerun
        return pend

    def reseed(self, seed, calls=0):
        """The training-mode forward's sampler: ``hip_train_seed`` and the call counter ``train_calls`` (the ``step`` of the next call)"""
        self.train_seed, self.train_calls = int(seed), int(calls)

    def _enqueue_training(self, data, feat_c, feat_f, fi, main, fkey, want_fine_debug, host_copy, _pe_applied):
        """The training-mode forward (``hip_train_forward``; OnePosePlusModel.py:95-203 with ``self.training``): the stages of the eval
        forward, all on the current stream (``hip_overlap_fine`` is ignored, the frame call never used), ``conf_matrix`` stored (the loss
        reads it), the coarse stage with its whole selection, and with ``coarse_matching.train.train_padding`` the reference's cut and GT
        padding (coarse_matching.py:174-217) into buffers of the host-known capacity ``T``, over which the fine stage then runs.  Without
        the padding the eval lists are returned as they are."""
        if "mask0" in data:
            raise NotImplementedError("data['mask0']: not implemented (the reference raises as well, coarse_matching.py:149-152)")
        if fkey in self._frame_call_pending:                          # order this frame's encoder behind the C path's last fine stage
            self._frame_call_pending.discard(fkey)
            hip.call("ophip_frame_order_after_fine", ctypes.c_void_p(main.cuda_stream))
        step, self.train_calls = self.train_calls, self.train_calls + 1
        x2d, x3d, ff, ff_strides = self._input_stage(fi, feat_c, feat_f, main, fkey, _pe_applied, False)
        layer_inputs = [] if self.keep_layer_inputs else None
        x3d, x2d = self._coarse_encoder_stage(fi, x3d, x2d, main, fkey, layer_inputs)
        if layer_inputs is not None:
            data["layer_inputs_c"] = layer_inputs
        if self.debug:
            data["_feat3d_c"], data["_feat2d_c"] = x3d, x2d
        cb, _ = self._coarse_matching_stage(data, fi, x3d, x2d, main, False, overlap=False)
        padded = bool(self.config["coarse_matching"]["train"]["train_padding"])
        if padded:
            cb = self._train_padding_stage(data, fi, cb, step)
        pend = self._fine_stage(data, fi, cb, None, ff, ff_strides, main, fkey, want_fine_debug or self.keep_features, host_copy, overlap=False)
        pend.padded, pend.want_dbg = padded, want_fine_debug
        if self.keep_features:
            pend.kept = (x3d, x2d)
        return pend

    def _train_padding_stage(self, data, fi, cb, step):
        """``train_forward.pad_matches`` behind the coarse stage's buffers ``cb``, on the current stream -> the same dictionary over buffers of
        capacity ``T``.  The block the host reads back holds ``T``'s count, ``n_keep`` and ``status`` in its first 16 bytes."""
        B, N, M, dev = fi.B, fi.N, fi.M, fi.dev
        tr = self.config["coarse_matching"]["train"]
        T, G = train_forward.train_rows(B, N, M, tr["train_coarse_percent"]), int(tr["train_pad_num_gt_min"])
        gt = supervision._ground_truth_of(data)
        if tuple(gt.shape) != (B, N, M):
            raise ValueError(f"the ground truth is of [B, N, M] = {list(gt.shape)}, the frame of {[B, N, M]}")
        f32, i64 = dict(device=dev, dtype=torch.float32), dict(device=dev, dtype=torch.int64)
        rows = max(T, 1)
        blob, count, b_ids, mk3d, mk2d = _result_views(torch.empty(16 + 28 * rows, dtype=torch.uint8, device=dev), rows)
        n_keep, status = blob[8:12].view(torch.int32), blob[12:16].view(torch.int32)
        fine_on = bool(self.config["fine_matching"]["enable"])
        out = MatchLists(b_ids, torch.empty(rows, **i64), torch.empty(rows, **i64), torch.empty(rows, **f32), mk3d,
                         torch.empty(rows, 2, **f32) if fine_on else mk2d, b_ids, torch.empty(rows, device=dev, dtype=torch.bool), count)
        pred = MatchLists(cb["b_ids"], cb["i_ids"], cb["j_ids"], cb["mconf"], cb["mk3d"], cb["mkc"], None, None, cb["count"])
        done = train_forward.pad_matches(pred, gt, fi.kpts_d, T=T, G=G, seed=self.train_seed, step=step, w_c=fi.wc, scale=data["q_hw_i"][0] / fi.hc,
                                         query_scale=fi.qscale, out=out, n_keep=n_keep, status=status)
        return dict(blob=blob, b_ids=out.b_ids, i_ids=out.i_ids, j_ids=out.j_ids, mconf=out.mconf, mk3d=mk3d, mk2d=mk2d, mkc=out.mkc, count=count,
                    m_bids=out.b_ids, gt_mask=out.gt_mask, cap=rows, held=(*cb["held"], cb, done))

    def _frame_inputs(self, data, feat_c, feat_f, image_hw):
        """Check one call's inputs and gather them as a :class:`FrameInputs`; fills the ``bs`` / ``q_hw_*`` keys of ``data``."""
        if not feat_c.is_cuda:
            raise hip.HipLibraryError("OnePosePlus_model runs on the HIP device only (no CPU fallback): move the "
                                      "model and its inputs to 'cuda'")
        if self.coarse_full and "query_image_mask" in data:
            if "cross" in self.loftr_coarse.layer_names:
                # the reference's masked full attention never completes: its 3D stream's cross layer passes x_mask=None with a source
                # mask, and FullAttention evaluates q_mask[:, :, None, None] on that None (linear_attention.py:85)
                raise TypeError("'NoneType' object is not subscriptable: query_image_mask with loftr_coarse.attention = 'full' "
                                "(the reference's FullAttention indexes the None q_mask of the 3D stream's cross layer, linear_attention.py:85)")
            raise NotImplementedError("query_image_mask with loftr_coarse.attention = 'full'")
        hip.load()
        dev = feat_c.device
        if image_hw is not None:
            data.update({"bs": feat_c.size(0), "q_hw_i": torch.Size(image_hw)})
        B, _, hc, wc = feat_c.shape
        hf, wf = feat_f.shape[2:]
        M = hc * wc
        data.update({"q_hw_c": feat_c.shape[2:], "q_hw_f": feat_f.shape[2:]})
        W = self._weights(dev)
        kpts = data["keypoints3d"]
        desc_fine = data["descriptors3d_db"]
        desc_in = data["descriptors3d_coarse_db"] if "descriptors3d_coarse_db" in data else desc_fine
        N = kpts.shape[1]
        kpts_d, desc_in_d, desc_fine_d = _per_frame(kpts), _per_frame(desc_in), _per_frame(desc_fine)
        for t, name in ((kpts_d, "keypoints3d"), (desc_in_d, "descriptors3d"), (desc_fine_d, "descriptors3d_db")):
            if t.shape[0] not in (1, B):
                raise ValueError(f"{name}: batch {t.shape[0]} does not match the query batch {B}")

        # optional inputs of padded / resized query images (OnePosePlusModel.py:104,156-158; datasets with img_pad / img_resize)
        qmask = qscale = None
        if "query_image_mask" in data:
            qm = data["query_image_mask"]
            if tuple(qm.shape) != (B, hc, wc):
                raise ValueError(f"query_image_mask: expected shape {(B, hc, wc)} (the coarse grid), got {tuple(qm.shape)}")
            qmask = (qm if qm.dtype == torch.bool else qm != 0).to(dev).contiguous().view(torch.uint8).view(B, M)
        if "query_image_scale" in data:
            qs = data["query_image_scale"]
            if tuple(qs.shape) != (B, 2):
                raise ValueError(f"query_image_scale: expected shape {(B, 2)} ((h, w) factors per image), got {tuple(qs.shape)}")
            qscale = qs.to(device=dev, dtype=torch.float32).contiguous()
        return FrameInputs(B, N, M, hc, wc, hf, wf, dev, kpts_d, desc_in_d, desc_fine_d, qmask, qscale, W)

    def _input_stage(self, fi, feat_c, feat_f, main, fkey, _pe_applied, inputs_ready):
        """Rows a1-a3 and the fine map's transpose -> ``(x2d [B, M, C], x3d [B, N, C], ff, ff_strides)`` (``ff`` None with the fine stage off).
        They depend on nothing but the caller's tensors.  With ``inputs_ready`` the caller states that those are complete (no producer still
        queued on this stream): the kernels then go to a side stream and start at once -- on the CUs the 246-workgroup encoder of the previous
        frame leaves idle and beside its coarse stage -- instead of behind everything queued before; the compute stream waits for their event."""
        B, N, M, hf, wf, dev = fi.B, fi.N, fi.M, fi.hf, fi.wf, fi.dev
        C = feat_c.shape[1]
        f32 = dict(device=dev, dtype=torch.float32)
        prep_ctx, sprep = contextlib.nullcontext(), None
        if inputs_ready and self.overlap_fine and not _pe_applied:
            sprep = _side_stream(self._prep_streams, fkey, dev)
            prep_ctx = torch.cuda.stream(sprep)
        with prep_ctx:                   # the launches below go to the stream that is current in here
            # ---- a1: positional encoding + flatten ------------------------------------------------
            if _pe_applied:          # the HIP backbone wrote [B, M, C] with the encoding added; the encoder may reuse that buffer
                x2d = feat_c.permute(0, 2, 3, 1).reshape(B, M, C)
                if x2d.data_ptr() != feat_c.data_ptr() or not x2d.is_contiguous():
                    raise ValueError("internal: the HIP backbone's coarse map must be dense channels-last")
            else:
                x2d = torch.empty(B, M, C, **f32)
                pe = self._pe_table(fi.hc, fi.wc, dev) if self._pe_enable else None
                hip.launch("ophip_pe_add_transpose", dict(feat_nchw=_dense(feat_c), pe_nlc=pe, out_nlc=x2d, B=B, C=C, M=M))
            # ---- fine map to channels-last (input kernel of the fine stage; here so that it runs under the previous frame's
            #      fine stage instead of in front of this frame's) ------------------------------------------------------
            ff = ff_strides = None
            if bool(self.config["fine_matching"]["enable"]):
                ff = feat_f if feat_f.dtype == torch.float32 else feat_f.float()
                if ff.stride(1) == 1:                      # channels-last memory already: strides as they are
                    ff_strides = (ff.stride(0), 1, ff.stride(2), ff.stride(3))
                else:                                      # NCHW: one streaming transpose, then every window pixel is a 512-byte row
                    ff = ff.contiguous()
                    ff_cl = torch.empty(B, hf * wf, ff.shape[1], **f32)
                    hip.launch("ophip_transpose_cl", dict(in_bcl=ff, out_blc=ff_cl, B=B, C=ff.shape[1], L=hf * wf))
                    ff, ff_strides = ff_cl, (hf * wf * ff_cl.shape[2], 1, wf * ff_cl.shape[2], ff_cl.shape[2])
            # ---- a2 + a3: keypoint encoding (frame-invariant: depends on the object block only) -------------------
            if self.cache_object:
                # the reference keeps the object block resident across frames (OnePosePlus_inference_dataset.py:157-169); its encoding
                # is recomputed only when the tensors (or the weights) change
                ent = self._object_cache_entry(fi, torch.cuda.current_stream(dev))
                torch.cuda.current_stream(dev).wait_event(ent["ev"])
                x3d = ent["x3d"] if ent["x3d"].shape[0] == B else ent["x3d"].expand(B, -1, -1).contiguous()
            else:
                x3d = self._encode_keypoints(fi, B)
            if sprep is not None:
                prep_done = torch.cuda.Event()
                prep_done.record()
        if sprep is not None:
            main.wait_event(prep_done)
            for t in (x2d, x3d, ff):                     # allocated from s_prep's pool, used on the compute / fine streams from here on
                if t is not None:
                    t.record_stream(main)
        return x2d, x3d, ff, ff_strides

    def _encode_keypoints(self, fi, Bo):
        """Rows a2 + a3 on the current stream: the object block's keypoint encoding ``[Bo, N, 256]``; ``Bo`` = 1 for one object shared by
        the batch, else B."""
        kpts_d, desc_in_d = fi.kpts_d, fi.desc_in_d
        x3d = torch.empty(Bo, fi.N, 256, device=fi.dev, dtype=torch.float32)
        if self.kpt_3d_pos_encoding is not None:
            stats = torch.empty(4 * Bo + 4, device=fi.dev, dtype=torch.float32)
            hip.launch("ophip_kpt_encode", dict(keypoints3d=kpts_d, kpts_bstride=bstride(kpts_d), desc_bcn=desc_in_d,
                                                desc_bstride=bstride(desc_in_d), wpack=fi.W["kpt"], stats=stats, out_bnc=x3d, B=Bo, N=fi.N))
        else:
            src = desc_in_d if desc_in_d.shape[0] == Bo else desc_in_d.expand(Bo, -1, -1).contiguous()
            hip.launch("ophip_transpose_cl", dict(in_bcl=src, out_blc=x3d, B=Bo, C=256, L=fi.N))
        return x3d

    def _coarse_layer_launch(self, fi, S, rows):
        """The coarse encoder layer in this model's arithmetic mode: ``launch(li, name, x3d, x2d, y3d, y2d)`` runs layer ``li`` (``name``
        "self" or "cross") from the x rows into the y rows on stream ``S`` (a ``torch.cuda.Stream``).  A mode is its workspace, weight
        blocks and whether its layers chain.  The entry and what a frame's layers share are planned once, here, from the first layer's
        ``rows`` (x3d, x2d, y3d, y2d); a call sets its own rows, weights and chain state (the staged path's host cost, section 6q)."""
        # "f32": exact (csrc/encoder.hip); "full": softmax attention -- projections, split-bf16 flash attention, tail (csrc/encoder_full.hip;
        # its entry point takes no mask); both read the f32 layer block.  "bf16x3": 16-token tiles, one eight-wave workgroup per CU, per-wave
        # weight streams (csrc/encoder_x3w8.hip); "bf16": the plain-bf16 kernel.  In the last two, layer li's attn_apply also emits layer
        # li+1's K/V partial slabs from the on-chip output tile.
        mode = "full" if self.coarse_full and self.precision != "f32" else self.precision
        Wl = fi.W[{"f32": "coarse", "full": "coarse", "bf16x3": "coarse_x3", "bf16": "coarse_bf16"}[mode]]
        last = len(self.loftr_coarse.layer_names) - 1
        entry, named = layercall.plan_layer(*rows, mode=mode, wpack=None, is_cross=0, workspace=layercall.workspace(mode, fi.B, fi.N, fi.M, fi.dev),
                                            query_mask=None if mode == "full" else fi.qmask)
        chained = "slot" in named

        def launch(li, name, x3d, x2d, y3d, y2d):
            named.update(x3d=x3d, x2d=x2d, y3d=y3d, y2d=y2d, wpack=Wl[li], is_cross=1 if name == "cross" else 0)
            if chained:
                named.update(wpack_next=Wl[li + 1] if li < last else None, kv_from_prev=1 if li > 0 else 0, slot=li & 1)
            hip.launch(entry, named, S)
        return launch

    def _coarse_encoder_stage(self, fi, x3d, x2d, main, fkey, layer_inputs=None):
        """Rows a4-a6 on the compute stream: the coarse encoder's layers over the 3D rows ``x3d`` and the 2D rows ``x2d``; returns the
        final ``(x3d, x2d)``.  It starts once the previous frame's fine stage is done: the two MFMA-heavy stages (attn_apply is the
        roofline kernel) never share the chip.  ``layer_inputs`` (a list; the training-mode forward with ``hip_keep_layer_inputs``): every
        layer's ``(x3d, x2d)`` is appended and no buffer is written twice."""
        names = self.loftr_coarse.layer_names
        y3d, y2d = torch.empty_like(x3d), torch.empty_like(x2d)
        z3d = torch.empty_like(x3d) if self.cache_object and layer_inputs is None else x3d      # (kept layer inputs: never used)
        prev = self._fine_streams.get(fkey)
        if (names or self.precision == "f32") and self.overlap_fine and prev is not None and prev[1] is not None:
            main.wait_event(prev[1])          # (the exact-f32 mode waits with no layer to run as well)
        launch = self._coarse_layer_launch(fi, main, (x3d, x2d, y3d, y2d))
        for li, name in enumerate(names):
            launch(li, name, x3d, x2d, y3d, y2d)
            if layer_inputs is not None:      # the inputs stay as they are: the next layer reads these outputs and writes fresh buffers
                layer_inputs.append((x3d, x2d))
                x3d, x2d = y3d, y2d
                if li < len(names) - 1:
                    y3d, y2d = torch.empty_like(x3d), torch.empty_like(x2d)
                continue
            # Ping-pong: the layer's outputs become the next layer's inputs, its inputs the next outputs.  The one invariant of this
            # function: a cached ``x3d`` (``hip_cache_object``: the object's entry, shared with later frames) is never an output buffer --
            # after layer 0 the 3D stream alternates between ``y3d`` and ``z3d``, which is a buffer of this frame's own when the encoding
            # is cached and the frame's own ``x3d`` otherwise.
            x3d, y3d, x2d, y2d = y3d, (z3d if li == 0 else x3d), y2d, x2d
        return x3d, x2d

    def _coarse_matching_stage(self, data, fi, x3d, x2d, main, lazy, overlap=None):
        """Rows a7 + a8 on the compute stream; sets ``data["conf_matrix"]``.  Returns the stage's buffers (read-only from here on; ``held``: what
        must stay referenced until ``finish()``) and ``select``: with the fine stage on its side stream the single-workgroup select kernel goes there with it (it only feeds that stage
        and the read-back: the next frame's input kernels then run beside it, not behind it) -- ``select(stream)`` launches it; else None."""
        B, N, M, dev, kpts_d, qmask, qscale = fi.B, fi.N, fi.M, fi.dev, fi.kpts_d, fi.qmask, fi.qscale
        f32, i64 = dict(device=dev, dtype=torch.float32), dict(device=dev, dtype=torch.int64)
        cm = self.config["coarse_matching"]
        cap = B * N
        conf = None if lazy else torch.empty(B, N, M, **f32)
        cws = torch.empty(hip.load().ophip_coarse_workspace_floats(B, N, M), **f32)
        # what the host reads back (count, b_ids, 3D points, refined 2D points) lives in one block: one D2H copy per frame
        blob, count, b_ids, mk3d, mk2d = _result_views(torch.empty(16 + 28 * cap, dtype=torch.uint8, device=dev), cap)
        i_ids, j_ids, m_bids = torch.empty(cap, **i64), torch.empty(cap, **i64), torch.empty(cap, **i64)
        gt_mask = torch.empty(cap, device=dev, dtype=torch.bool)
        fine_on = bool(self.config["fine_matching"]["enable"])
        mconf = torch.empty(cap, **f32)
        mkc = torch.empty(cap, 2, **f32) if fine_on else mk2d
        scale = data["q_hw_i"][0] / fi.hc
        temperature = float(cm["dual_softmax"]["temperature"])
        lists = MatchLists(b_ids, i_ids, j_ids, mconf, mk3d, mkc, m_bids, gt_mask, count)
        split_select = fine_on and (self.overlap_fine if overlap is None else overlap)      # (the training-mode forward: all on one stream)

        def match(parts, stream):
            coarse_match(x3d, x2d, kpts_d, wc=fi.wc, temperature=temperature, thr=cm["thr"], border_rm=cm["border_rm"], scale=scale,
                         nsplit=_NSPLIT[self.precision], lists=lists, conf=conf, workspace=cws, parts=parts, query_mask=qmask,
                         query_scale=qscale, stream=stream)
        with self.profiler.record_function("LoFTR/coarse-matching/get_coarse_match"):
            match(1 if split_select else 3, main)
        select = (lambda stream: match(2, stream)) if split_select else None
        data["conf_matrix"] = conf if not lazy else LazyConfMatrix(x3d, x2d, temperature, _NSPLIT[self.precision], main, qmask)
        return dict(blob=blob, b_ids=b_ids, i_ids=i_ids, j_ids=j_ids, mconf=mconf, mk3d=mk3d, mk2d=mk2d, mkc=mkc, count=count, m_bids=m_bids,
                    gt_mask=gt_mask, held=(x3d, x2d, cws, conf)), select

    def _fine_stage(self, data, fi, cb, select, ff, ff_strides, main, fkey, want_fine_debug, host_copy, overlap=None):
        """Rows a9-a11 on the coarse stage's buffers ``cb`` (behind the kept-back selection ``select``) and the frame's :class:`PendingFrame`.  With ``hip_overlap_fine`` they run on
        the compute stream's fine stream, behind an event of the coarse stage, and leave the event the next frame's encoder waits for.  The grid
        is sized by the capacity B * N (one match per 3D point at most; surplus workgroups exit on the device-side count): no sync yet."""
        B, N, M, hf, dev, desc, qscale, W = fi.B, fi.N, fi.M, fi.hf, fi.dev, fi.desc_fine_d, fi.qscale, fi.W
        cfg = self.config
        fine_on = bool(cfg["fine_matching"]["enable"])
        f32 = dict(device=dev, dtype=torch.float32)
        cap = cb.get("cap", B * N)                    # (the training-mode forward's padded lists: T)
        fine_ctx, fine_entry = contextlib.nullcontext(), None
        if fine_on and (self.overlap_fine if overlap is None else overlap):
            fine_entry = _side_stream(self._fine_streams, fkey, dev, with_event=True)
            coarse_done = torch.cuda.Event()
            coarse_done.record(main)
            fine_entry[0].wait_event(coarse_done)
            fine_ctx = torch.cuda.stream(fine_entry[0])
        keep = [desc, W, fi.qmask, qscale, ff, *cb["held"]]          # inputs of the side-stream kernels stay referenced until finish()
        expec = dbg_w = dbg_3 = None
        with fine_ctx:
            if select is not None:
                select(None)                              # on the stream of this context
            if fine_on:
                cf = cfg["loftr_fine"]
                expec = torch.empty(cap, 3, **f32)
                dbg_w = torch.empty(cap, 25, 128, **f32) if want_fine_debug else None
                dbg_3 = torch.empty(cap, 128, **f32) if want_fine_debug else None
                names_f = self.loftr_fine.layer_names
                cross_bits = sum(1 << i for i, n in enumerate(names_f) if n == "cross")
                stride = hf // fi.hc
                if self.fine_full:
                    fw, fd3 = self._fine_full_stage(fi, cb, ff, ff_strides, stride, float(data["q_hw_i"][0] / hf), expec)
                    if want_fine_debug:
                        dbg_w, dbg_3 = fw, fd3
                else:
                    bf = self.precision != "f32"          # the bf16 pipe's kernel takes its operand split (3: split-bf16, 1: plain) as well
                    fine_scale = (cf["window_size"] // 2) * (data["q_hw_i"][0] / hf)
                    fine_refine(ff, ff_strides, hf, fi.wf, desc, b_ids=cb["b_ids"], i_ids=cb["i_ids"], j_ids=cb["j_ids"], count=cb["count"],
                                mkpts_c=cb["mkc"], max_matches=cap, wpack=W["fine_bf16"] if bf else W["fine"], nlayers=len(names_f),
                                cross_bits=cross_bits, encoder_enable=1 if cf["enable"] else 0, nsplit=_NSPLIT[self.precision] if bf else None,
                                wc=fi.wc, stride=stride, fine_scale=fine_scale, expec_f=expec, mkpts_f=cb["mk2d"], dbg_win=dbg_w, dbg_f3=dbg_3,
                                query_scale=qscale)
            if fine_entry is not None:
                fine_done = torch.cuda.Event()
                fine_done.record()
                fine_entry[1] = fine_done
            bufs = dict(blob=cb["blob"], b_ids=cb["b_ids"], i_ids=cb["i_ids"], j_ids=cb["j_ids"], mconf=cb["mconf"], mk3d=cb["mk3d"], mkc=cb["mkc"],
                        count=cb["count"], m_bids=cb["m_bids"], gt_mask=cb["gt_mask"], expec=expec, mkf=cb["mk2d"] if fine_on else None,
                        dbg_w=dbg_w, dbg_3=dbg_3, keep=keep)
            return PendingFrame(self, data, dev, B, N, M, cap, fine_on, want_fine_debug, bufs, host_copy)

    def _fine_full_stage(self, fi, cb, ff, ff_strides, stride, scale, expec):
        """Rows a9-a11 with the fine encoder's full attention, on the current stream: gather (window and 3D token rows), the encoder layers
        (transformer.py:133-171 on [K, 1, C] 3D tokens and [K, 25, C] windows; a cross layer's 3D update reads the pre-update windows), then
        FineMatching on the one 3D token per match into ``expec`` and ``cb["mk2d"]``.  Every row count is the capacity: the kernels read the device-side count.  Returns the
        encoder's output rows (windows [cap, 25, 128], 3D tokens [cap, 128])."""
        f32 = dict(device=fi.dev, dtype=torch.float32)
        desc, cap, cnt = fi.desc_fine_d, cb.get("cap", fi.B * fi.N), cb["count"]
        WS, WW = 5, 25
        win, f3 = torch.empty(cap, WW, 128, **f32), torch.empty(cap, 128, **f32)
        hip.launch("ophip_fine_full_gather", dict(zip(("fs_b", "fs_c", "fs_y", "fs_x"), ff_strides), feat_f=ff, hf=fi.hf, wf=fi.wf, desc3d_f=desc,
                                                  d_bs=bstride(desc), d_cs=desc.stride(1), b_ids=cb["b_ids"], i_ids=cb["i_ids"],
                                                  j_ids=cb["j_ids"], count=cnt, cap=cap, wc=fi.wc, stride=stride, W=WS, windows=win, feat3d=f3))

        def layer(x, Lx, src, Ls, w):                     # LoFTREncoderLayer with FullAttention over each match's Lx x Ls tokens
            return rows_encoder_layer(x, cap * Lx, src, cap * Ls, w, lambda q, k, v, msg: hip.launch(
                "ophip_fine_full_attention", dict(q=q, k=k, v=v, K=cap, L=Lx, S=Ls, count=cnt, msg=msg)))
        if bool(self.config["loftr_fine"]["enable"]):
            for w, name in zip(fi.W["fine_full"], self.loftr_fine.layer_names):
                if name == "self":
                    win, f3 = layer(win, WW, win, WW, w), layer(f3, 1, f3, 1, w)
                else:
                    win, f3 = layer(win, WW, f3, 1, w), layer(f3, 1, win, WW, w)
        hip.launch("ophip_fine_full_match", dict(feat3d=f3, windows=win, mkpts_c=cb["mkc"], b_ids=cb["b_ids"], query_scale=fi.qscale, count=cnt,
                                                 cap=cap, W=WS, scale=scale, expec_f=expec, mkpts_f=cb["mk2d"]))
        return win, f3

    def _object_cache_entry(self, fi, stream, masked=False, keep=True):
        """The object's cache entry ``{"x3d", "y3d0", "kv1", "ev"}`` (``ophip_object_cache``), built on a miss on ``stream`` with the kernels a
        frame would run.  Keyed on the object tensors' storage + version and the packed weights; ``Bo`` = 1 rows when the batch shares one
        object block (stride-0 expand / batch-1 tensors under a larger query batch), else B."""
        B, N, dev, kpts_d, desc_in_d, W = fi.B, fi.N, fi.dev, fi.kpts_d, fi.desc_in_d, fi.W
        Bo = 1 if (B > 1 and kpts_d.shape[0] == 1 and desc_in_d.shape[0] == 1) else B
        names = self.loftr_coarse.layer_names
        deep = (self.precision == "bf16x3" and not self.coarse_full and not self.fine_full and len(names) >= 2 and names[0] == "self"
                and os.environ.get("OPHIP_OBJECT_CACHE_DEPTH", "2") != "1")
        # (masked: frames with a query_image_mask run both streams through the masked instantiation of the layer kernel; their entry is built
        #  with that instantiation, see ophip_encoder_object_x3w8)
        ckey = (str(dev), Bo, N, kpts_d.data_ptr(), kpts_d._version, desc_in_d.data_ptr(), desc_in_d._version, id(W), deep, bool(masked) and deep)
        ent = self._obj_cache
        if keep and ent is not None and ent["key"] == ckey:
            return ent
        with torch.cuda.stream(stream):
            x3d = self._encode_keypoints(fi, Bo)
            y3d0 = kv1 = None
            if deep:
                y3d0 = torch.empty(Bo, N, 256, device=dev, dtype=torch.float32)
                kv1 = torch.empty(Bo, layercall.kv_block_bytes(), device=dev, dtype=torch.uint8)
                layercall.object_rows(x3d, wpack0=W["coarse_x3"][0], wpack1=W["coarse_x3"][1], workspace=layercall.workspace("bf16x3", Bo, N, 1, dev),
                                      y3d0=y3d0, kv1=kv1, masked_frames=1 if masked else 0)
            ev = torch.cuda.Event()
            ev.record(stream)
        ent = {"key": ckey, "x3d": x3d, "y3d0": y3d0, "kv1": kv1, "ev": ev, "keep": (kpts_d, desc_in_d, W)}      # the key's tensors stay alive with the entry
        if keep:
            self._obj_cache = ent
        return ent

    def flush(self):
        """End of a sequence: no further frame is coming on the current stream, so the last frame's kept-back fine stage (it would otherwise
        go out with the next ``enqueue`` or at its ``finish()``) is launched now, behind its own selection.  Optional -- ``finish()`` does it
        as well, only later (after the frames before it have been waited for)."""
        dev = torch.cuda.current_device()
        main = torch.cuda.current_stream()
        fkey = (str(torch.device("cuda", dev)), main.cuda_stream)
        if fkey in self._frame_call_pending:
            hip.call("ophip_frame_order_after_fine", ctypes.c_void_p(main.cuda_stream))

    def _frame_plan(self, fi, cf_ch, transpose_fine, ext_mode, img_h, lazy):
        """``(desc, layout, plan id, kept tensors)`` of ``ophip_frame_enqueue`` for this input shape: built and registered once, then looked up"""
        B, N, M, hc, wc, hf, wf, dev, W = fi.B, fi.N, fi.M, fi.hc, fi.wc, fi.hf, fi.wf, fi.dev, fi.W
        pkey = (str(dev), B, N, M, hc, wc, hf, wf, cf_ch, bool(transpose_fine), ext_mode, int(img_h), id(W), bool(lazy))
        plan = self._frame_plans.get(pkey)
        if plan is None:
            cm, lf = self.config["coarse_matching"], self.config["loftr_fine"]
            d = hip.FrameDesc()
            d.B, d.N, d.M, d.hc, d.wc, d.hf, d.wf, d.cf = B, N, M, hc, wc, hf, wf, cf_ch
            d.lazy_conf = 1 if lazy else 0
            names_c, names_f = self.loftr_coarse.layer_names, self.loftr_fine.layer_names
            d.n_coarse, d.coarse_cross_bits = len(names_c), sum(1 << i for i, n in enumerate(names_c) if n == "cross")
            d.n_fine, d.fine_cross_bits = len(names_f), sum(1 << i for i, n in enumerate(names_f) if n == "cross")
            d.fine_encoder_enable = 1 if lf["enable"] else 0
            d.border_rm = int(cm["border_rm"])
            d.thr, d.scale_c = float(cm["thr"]), float(img_h / hc)
            d.fine_scale = float((lf["window_size"] // 2) * (img_h / hf))
            d.temperature = float(cm["dual_softmax"]["temperature"])
            pe = self._pe_table(hc, wc, dev) if self._pe_enable else None
            d.pe = pe.data_ptr() if pe is not None else None
            d.w_kpt = W["kpt"].data_ptr() if self.kpt_3d_pos_encoding is not None else None
            for li in range(len(names_c)):
                d.w_coarse[li] = W["coarse_x3"][li].data_ptr()
            d.w_fine = W["fine_bf16"].data_ptr()
            L = hip.FrameLayout()
            hip.call("ophip_frame_layout", ctypes.byref(d), 1 if transpose_fine else 0, ext_mode, ctypes.byref(L))
            if len(self._frame_plans) >= 8:
                old_id = self._frame_plans.pop(next(iter(self._frame_plans)))[2]
                self._plan_ids.discard(old_id)
                ops.drop_frame_plan(old_id)
            pid = ops.register_frame_plan(d, L, keep_alive=(W, pe))
            self._plan_ids.add(pid)
            plan = self._frame_plans[pkey] = (d, L, pid, (W, pe))      # W and the table stay alive with the pointers, here and in the registry
        return plan

    def _enqueue_frame_call(self, data, feat_c, feat_f, fi, main, fkey, host_copy, inputs_ready, lazy=False, rerun=None):
        """The whole frame through ``ophip_frame_enqueue`` (csrc/frame.hip): one device block, one C call."""
        B, N, M, dev, kpts_d, desc_in_d, desc_fine_d, qmask, qscale = fi.B, fi.N, fi.M, fi.dev, fi.kpts_d, fi.desc_in_d, fi.desc_fine_d, fi.qmask, fi.qscale
        x3d_ext = None
        if self.cache_object or (B > 1 and kpts_d.shape[0] == 1 and desc_in_d.shape[0] == 1):
            # the reference keeps the object block resident across frames (OnePosePlus_inference_dataset.py:157-169): what depends on it
            # and the weights alone is computed once per (object tensors, weights) and handed to the frame call -- the keypoint encoding
            # (rows a2 + a3) and, with a first layer of kind "self", that layer's 3D rows and the K^T V | Ksum block of those rows as the
            # second layer's source (transformer.py:148-159; ophip_encoder_object_x3w8: the frame's own launches on the 3D stream's
            # workgroups, so a cached frame is bit-identical).  One entry serves the whole batch when it shares one object (config 3).
            # A batch whose frames share ONE object block (stride-0 expand: BASELINE config 3) takes the same route WITHOUT the cache flag:
            # the object-only work is then done once per CALL instead of once per frame of the batch -- nothing is kept for the next call
            # (`keep=False`), so a forward still does all of its own work.
            x3d_ext = self._object_cache_entry(fi, main, masked=qmask is not None, keep=self.cache_object)
        fc = _dense(feat_c)
        ff = feat_f if feat_f.dtype == torch.float32 else feat_f.float()
        transpose_fine = ff.stride(1) != 1
        if transpose_fine:
            ff = ff.contiguous()
        ext_mode = 0 if x3d_ext is None else (2 if x3d_ext["y3d0"] is not None else 1)      # ophip_frame_layout's external_x3d
        d, L, plan_id = self._frame_plan(fi, ff.shape[1], transpose_fine, ext_mode, data["q_hw_i"][0], lazy)[:3]

        fine_entry = self._fine_streams.get(fkey)
        if fine_entry is None:                     # (only this path reads OPHIP_FINE_PRIO: the stage-by-stage path's fine stream has the default priority)
            fine_entry = _side_stream(self._fine_streams, fkey, dev, int(os.environ.get("OPHIP_FINE_PRIO", "0")), with_event=True)
        elif fine_entry[1] is not None:            # a stage-by-stage frame before this one: order behind its fine stage
            main.wait_event(fine_entry[1])
            fine_entry[1] = None
        sfine = fine_entry[0]
        sprep = _side_stream(self._prep_streams, fkey, dev) if inputs_ready else None
        scopy = _side_stream(PendingFrame._copy_streams, (dev, main.cuda_stream), dev)
        cap = B * N
        if sprep is not None:
            # the input kernels write into the block on s_prep AHEAD of everything queued on the compute stream, so the block must come
            # from s_prep's pool (the caching allocator orders reuse on the allocating stream only: a block freed on the compute stream
            # with work still pending there could otherwise be overwritten early); the other streams that touch it are recorded, so
            # that it goes back to the pool only after their work is done
            with torch.cuda.stream(sprep):
                blob = torch.empty(L.total, dtype=torch.uint8, device=dev)
        else:
            blob = torch.empty(L.total, dtype=torch.uint8, device=dev)
        for st in (sfine, scopy) if sprep is None else (main, sfine, scopy):
            blob.record_stream(st)
        nbytes = int(L.result_bytes) if host_copy else 16
        pin = PendingFrame._take_pin((cap, bool(host_copy)), nbytes)
        fs = (0, 0, 0, 0) if transpose_fine else (ff.stride(0), 1, ff.stride(2), ff.stride(3))      # zeros: the callee fills in its channels-last copy's
        try:
            # the whole frame through ONE custom op (torch.ops.onepose_hip.frame_enqueue -> ophip_frame_enqueue).  The reference's two
            # profiler scopes (coarse_matching.py:122,167) enclose it -- get_coarse_match and its argmax are inside this call; a profiler no
            # longer takes the model off the one-call path -- and the library adds a roctx range per stage and kernel (OPHIP_ROCTX=1).
            with self.profiler.record_function("LoFTR/coarse-matching/get_coarse_match"), \
                    self.profiler.record_function("LoFTR/coarse-matching/get_coarse_match/argmax-conf"):
                oc = x3d_ext or {"x3d": None, "y3d0": None, "kv1": None, "ev": None}
                slot = torch.ops.onepose_hip.frame_enqueue(plan_id, blob, fc, ff, list(fs), kpts_d, desc_in_d, desc_fine_d, oc["x3d"], pin, nbytes,
                                                           main.cuda_stream, sprep.cuda_stream if sprep is not None else 0,
                                                           sfine.cuda_stream, scopy.cuda_stream, qmask, qscale, oc["y3d0"], oc["kv1"],
                                                           oc["ev"].cuda_event if oc["ev"] is not None else 0)
        except Exception:
            # part of the frame may be queued on the side streams already: nothing may touch the block or the pinned buffer again
            # before those streams are idle
            torch.cuda.synchronize(dev)
            PendingFrame._pinned_pool.setdefault((cap, bool(host_copy)), []).append(pin)
            raise
        self._frame_call_pending.add(fkey)
        if lazy:
            f3 = blob[L.feat3d_out:L.feat3d_out + 4 * B * N * 256].view(torch.float32).view(B, N, 256)
            f2 = blob[L.feat2d_out:L.feat2d_out + 4 * B * M * 256].view(torch.float32).view(B, M, 256)
            data["conf_matrix"] = LazyConfMatrix(f3, f2, float(self.config["coarse_matching"]["dual_softmax"]["temperature"]), _NSPLIT["bf16x3"], main, qmask)
        else:
            data["conf_matrix"] = blob[L.conf:L.conf + 4 * B * N * M].view(torch.float32).view(B, N, M)
        keep = [fc, ff, kpts_d, desc_in_d, desc_fine_d, x3d_ext, fi.W, qmask, qscale]
        pend = PendingFrame._from_block(self, data, dev, B, N, M, cap, blob, L, slot, pin, host_copy, keep)
        pend._rerun = rerun
        return pend


class LazyConfMatrix(LazyConfMatrixBase):
    """``data["conf_matrix"]`` of the lazy form (``config["hip_conf_matrix"] = "lazy"``): the N x M dual-softmax matrix is not stored
    by the frame; this object keeps the encoder's final rows and computes it on first use -- same kernels, same bits as the eager
    form (``ophip_coarse_match_conf`` with a conf buffer).  ``shape`` / ``dtype`` / ``device`` answer without materialising; indexing,
    attribute access (``.max``, ``.cpu`` ...) and ``torch.*`` functions materialise first (``lazy_conf.LazyConfMatrixBase``, shared with
    the LoFTR matcher).  Reference: ``utils/coarse_matching.py:115``; its readers at inference time: none (``inference.py:179-180``)."""

    def __init__(self, feat3d, feat2d, temperature, nsplit, stream, query_mask=None):
        super().__init__((feat3d.shape[0], feat3d.shape[1], feat2d.shape[1]), feat3d.device)
        self._f3, self._f2, self._temp, self._nsplit, self._stream, self._qmask = feat3d, feat2d, temperature, nsplit, stream, query_mask

    def _compute(self) -> torch.Tensor:
        B, N, M = self.shape
        dev = self.device
        cur = torch.cuda.current_stream(dev)
        cur.wait_stream(self._stream)             # the frame's encoder has produced the rows
        conf = torch.empty(B, N, M, device=dev, dtype=torch.float32)
        ws = torch.empty(hip.load().ophip_coarse_workspace_floats(B, N, M), device=dev, dtype=torch.float32)
        cap = B * N
        ids = torch.empty(3 * cap, dtype=torch.int64, device=dev)
        fl = torch.empty(6 * cap + 3, dtype=torch.float32, device=dev)
        cnt = torch.zeros(4, dtype=torch.int32, device=dev)
        lists = MatchLists(ids[:cap], ids[cap:2 * cap], ids[2 * cap:], fl[3:3 + cap], fl[3 + cap:3 + 4 * cap], fl[3 + 4 * cap:3 + 6 * cap], None, None, cnt)
        coarse_match(self._f3, self._f2, fl[:3], kpts_bstride=0, wc=M, temperature=self._temp, thr=0.5, border_rm=0, scale=1.0,
                     nsplit=self._nsplit, lists=lists, conf=conf, workspace=ws, parts=1, query_mask=self._qmask)
        self._f3 = self._f2 = None
        return conf


def _result_views(blob, cap):
    """(blob, count int32[1], b_ids int64[cap], mkpts3d f32[cap,3], mkpts2d f32[cap,2]) views of one byte block."""
    o_b, o_3, o_2 = 16, 16 + 8 * cap, 16 + 20 * cap
    return (blob, blob[:4].view(torch.int32), blob[o_b:o_3].view(torch.int64),
            blob[o_3:o_2].view(torch.float32).view(cap, 3), blob[o_2:o_2 + 8 * cap].view(torch.float32).view(cap, 2))


class PendingFrame:
    """A batch whose kernels are enqueued but whose match count has not been read yet."""

    _pinned_pool = {}
    _copy_streams = {}          # (device, compute stream) -> side stream for the result read-back

    def __init__(self, model, data, dev, B, N, M, cap, fine_on, want_dbg, bufs, host_copy):
        self.model, self.data, self.dev = model, data, dev
        self.B, self.N, self.M, self.cap, self.fine_on, self.want_dbg = B, N, M, cap, fine_on, want_dbg
        self.bufs = bufs
        self.host = None
        key = (cap, bool(host_copy))
        nbytes = bufs["blob"].numel() if host_copy else 16
        self._pin = PendingFrame._take_pin(key, nbytes)
        self._key, self._host_copy = key, bool(host_copy)
        self._slot = None
        self._rerun = None
        self.padded = False         # the training-mode forward's padded lists: the block's first 16 bytes hold n_keep and status too
        self.kept = None            # hip_keep_features: the coarse encoder's outputs, written to data with the fine encoder's at finish()
        # the D2H of the result block runs on a side stream behind an event: on the compute stream the PCIe round trip
        # (~40 us per frame) would sit between this frame's last kernel and the next frame's first one
        main = torch.cuda.current_stream(dev)
        side = _side_stream(PendingFrame._copy_streams, (dev, main.cuda_stream), dev)
        ready = torch.cuda.Event()
        ready.record(main)
        side.wait_event(ready)
        self.event = torch.cuda.Event()
        with torch.cuda.stream(side):
            self._pin.copy_(bufs["blob"][:nbytes], non_blocking=True)      # bufs (kept until finish) outlive the copy
            self.event.record(side)
        self.done = False

    @staticmethod
    def _take_pin(key, nbytes):
        pool = PendingFrame._pinned_pool.setdefault(key, [])
        return pool.pop() if pool else torch.empty(nbytes, dtype=torch.uint8).pin_memory()

    @classmethod
    def _from_block(cls, model, data, dev, B, N, M, cap, blob, layout, slot, pin, host_copy, keep):
        """A frame enqueued by ``ophip_frame_enqueue``: outputs are views into its device block, made at ``finish()``."""
        self = cls.__new__(cls)
        self.model, self.data, self.dev = model, data, dev
        self.B, self.N, self.M, self.cap, self.fine_on, self.want_dbg = B, N, M, cap, True, False
        self.bufs, self.host = None, None
        self._block, self._layout, self._slot, self._keep = blob, layout, slot, keep
        self._pin, self._key, self._host_copy = pin, (cap, bool(host_copy)), bool(host_copy)
        self.event = None
        self._rerun = None
        self.padded = False
        self.kept = None
        self.done = False
        return self

    def wait(self):
        """Block until this frame's results (and its read-back) are complete; ``finish()`` calls it."""
        self._wait()

    def _wait(self):
        if self._slot is not None:
            hip.call("ophip_frame_wait", self._slot)
        else:
            self.event.synchronize()

    def _block_views(self):
        blob, L, cap = self._block, self._layout, self.cap
        res = blob[L.result:L.result + L.result_bytes]
        _, count, b_ids, mk3d, mk2d = _result_views(res, cap)

        def v(off, nbytes, dt):
            return blob[off:off + nbytes].view(dt)
        return dict(blob=res, b_ids=b_ids, i_ids=v(L.i_ids, 8 * cap, torch.int64), j_ids=v(L.j_ids, 8 * cap, torch.int64),
                    mconf=v(L.mconf, 4 * cap, torch.float32), mk3d=mk3d, mkc=v(L.mkc, 8 * cap, torch.float32).view(cap, 2), count=count,
                    m_bids=v(L.m_bids, 8 * cap, torch.int64), gt_mask=v(L.gt_mask, cap, torch.bool),
                    expec=v(L.expec, 12 * cap, torch.float32).view(cap, 3), mkf=mk2d, dbg_w=None, dbg_3=None, keep=self._keep)

    def _release_pin(self):
        if self._pin is not None:
            pool = PendingFrame._pinned_pool.setdefault(self._key, [])
            if len(pool) < 8:                       # a few frames in flight at most: do not hoard pinned memory
                pool.append(self._pin)
            self._pin = None

    def close(self):
        """Abandon the frame: wait until the side streams (fine stage, read-back) are done with its buffers, then release them.
        Called by ``__del__``, so a frame dropped without ``finish()`` (an exception in the pipeline) cannot hand device blocks
        that are still being read or written back to the caching allocator."""
        if self.done or self._pin is None:
            return
        try:
            self._wait()
        finally:
            self._release_pin()
            self.done = True

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def finish(self, on_host=None):
        """Wait for this frame (event), read K, fill ``data`` exactly like the reference's ``forward``.  ``on_host(host)``: called with the
        frame's host-side matches (``host_copy=True``: K, 3D points, refined 2D points, b_ids) as soon as they are read -- before the
        device-side views of ``data`` are made -- so that a pipeline hands them to its pose solver ~50 us earlier."""
        if self.done:
            return self.data
        self._wait()                                # the one host wait of the frame
        K = int(self._pin[:4].view(torch.int32)[0])
        if self._rerun is not None and int(self._pin[4:8].view(torch.int32)[0]) != 0:
            # lazy conf_matrix and an exact tie of a row maximum whose first column failed the mutual test: which column the reference
            # takes next can only be read from the stored row -> this frame again, eagerly (identical arithmetic, conf_matrix stored)
            self._release_pin()
            self.done = True
            self.model.lazy_reruns += 1
            again = self._rerun()
            again.finish(on_host)
            self.host = again.host
            return self.data
        B, N, M, cap = self.B, self.N, self.M, self.cap
        n_keep = K
        if self.padded:
            # coarse_matching.py:231-239, fine_matching.py:105: the ids, gt_mask and expec_f keep all T rows, the prediction's keys the
            # n_keep predicted rows
            n_keep, status = (int(v) for v in self._pin[8:16].view(torch.int32))
            if status == train_forward.NO_GT:
                self._release_pin()
                self.done = True
                raise ValueError("no ground-truth match in the batch")
        if self._host_copy:
            _, _, hb, h3, h2 = _result_views(self._pin, cap)
            self.host = {"K": n_keep, "mkpts_3d_db": h3[:n_keep].numpy().copy(), "mkpts_2d": h2[:n_keep].numpy().copy(), "b_ids": hb[:n_keep].numpy().copy()}
            if on_host is not None:
                on_host(self.host)
        self._release_pin()
        if self.bufs is None:
            self.bufs = self._block_views()
        bf = self.bufs
        data, dev = self.data, self.dev
        b_ids, i_ids, j_ids = bf["b_ids"][:K], bf["i_ids"][:K], bf["j_ids"][:K]
        mconf, mk3d, mkc = bf["mconf"][:n_keep], bf["mk3d"][:n_keep], bf["mkc"][:n_keep]
        data.update({
            "b_ids": b_ids, "i_ids": i_ids, "j_ids": j_ids,
            "gt_mask": bf["gt_mask"][:K], "m_bids": bf["m_bids"][:n_keep],
            "mkpts_3d_db": mk3d, "mkpts_query_c": mkc, "mconf": mconf,
        })
        self.done = True
        if self.kept is not None:
            data["feat_c0"], data["feat_c1"] = self.kept
            if self.fine_on:
                data["feat_f0"], data["feat_f1"] = bf["dbg_3"], bf["dbg_w"]      # every row of the capacity: rows past the count are not written
        if not self.fine_on:
            data.update({"mkpts_3d_db": data["mkpts_3d_db"], "mkpts_query_f": data["mkpts_query_c"]})
            return data
        data.update({"W": self.model.config["loftr_fine"]["window_size"]})
        if K == 0:
            data.update({"expec_f": torch.empty(0, 3, device=dev), "mkpts_3d_db": mk3d, "mkpts_query_f": mkc})
            return data
        data.update({"expec_f": bf["expec"][:K], "mkpts_3d_db": mk3d, "mkpts_query_f": bf["mkf"][:n_keep]})
        if self.want_dbg:
            data["_fine_win"], data["_fine_f3"] = bf["dbg_w"][:K], bf["dbg_3"][:K]
        return data


def build_model(model_configs, ckpt_path) -> OnePosePlus_model:
    """``src/inference/inference_OnePosePlus.py:30-40``: strip the ``matcher.`` prefix, strict
    load, eval.  The checkpoint is read with ``weights_only=True`` (nothing from the file is
    executed)."""
    model = OnePosePlus_model(model_configs)
    state_dict = torch.load(ckpt_path, map_location="cpu", weights_only=True)["state_dict"]
    return load_matcher_checkpoint(model, state_dict)
