"""``data["conf_matrix"]`` of the lazy form, the part that both matchers share.

With ``hip_conf_matrix = "lazy"`` neither :class:`onepose_st_amd.model.OnePosePlus_model` nor
:class:`onepose_st_amd.loftr.LoFTR_for_OnePose_Plus` stores the N x M dual-softmax matrix: inference callers read only the match lists.
``data["conf_matrix"]`` is then a :class:`LazyConfMatrixBase`: it answers ``shape`` / ``dtype`` / ``device`` without work and computes the
matrix on first real use -- indexing, attribute access (``.max``, ``.cpu`` ...) and ``torch.*`` functions (``__torch_function__``).  A
subclass keeps the encoder's final rows and says in ``_compute`` how the matrix is made from them: the eager form of the same entry
point, so the bits are the eager call's.
"""
from __future__ import annotations

import torch


class LazyConfMatrixBase:
    def __init__(self, shape, device):
        self._t = None
        self.shape = torch.Size(shape)
        self.dtype, self.device = torch.float32, device

    def _compute(self) -> torch.Tensor:
        """-> the ``shape`` float32 matrix; called once.  Drops what it kept alive for the purpose."""
        raise NotImplementedError

    def materialize(self) -> torch.Tensor:
        if self._t is None:
            self._t = self._compute()
        return self._t

    def size(self, dim=None):
        return self.shape if dim is None else self.shape[dim]

    def dim(self):
        return len(self.shape)

    def __len__(self):
        return self.shape[0]

    def __getitem__(self, idx):
        return self.materialize()[idx]

    def __getattr__(self, name):                      # anything a tensor has and this object does not: materialise, then delegate
        if name.startswith("_"):
            raise AttributeError(name)
        return getattr(self.materialize(), name)

    def __repr__(self):
        return f"{type(self).__name__}(shape={tuple(self.shape)}, materialised={self._t is not None})"

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        def conv(a):
            if isinstance(a, LazyConfMatrixBase):
                return a.materialize()
            if isinstance(a, (list, tuple)):
                return type(a)(conv(x) for x in a)
            return a
        return func(*conv(tuple(args)), **{k: conv(v) for k, v in (kwargs or {}).items()})
