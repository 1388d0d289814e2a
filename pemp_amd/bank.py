"""Prototype banks: the prototypes of K classes, enrolled once from their supports (``model.enroll``) and met by any
number of queries afterwards (``model.segment`` / ``segment_lowres`` / ``segment_graphed``).

The prototypes of the prototype-matching families -- PEMP stage 1 (meta-prototypes, or plain masked average pooling with
``protos = 0``), Baseline, PANet -- depend on the supports alone, so an episode's support passes through the trunk need not
be repeated for every query.  The bank keeps them in the layout the head kernels share (``[K, 2p, c]``, foreground rows
first) together with what a query pass must agree with: the model family, its backbone, the precision the trunk ran at,
``p``, ``c`` and ``dist_scalar``."""
import torch

_FIELDS = ("family", "backbone", "precision", "p", "c", "dist_scalar")


class PrototypeBank:
    def __init__(self, protos, family, backbone, precision, dist_scalar, labels=None):
        if protos.dim() != 3 or protos.dtype != torch.float32 or protos.shape[1] < 2 or protos.shape[1] % 2:
            raise ValueError(f"PrototypeBank: protos must be fp32 [K,2p,c], got {tuple(protos.shape)} {protos.dtype}")
        self.protos = protos.contiguous()
        self.family, self.backbone, self.precision = str(family), str(backbone), str(precision)
        self.p, self.c = int(protos.shape[1]) // 2, int(protos.shape[2])
        self.dist_scalar = float(dist_scalar)
        self.labels = self._labels(labels, len(self))

    @staticmethod
    def _labels(labels, k):
        if labels is None:
            return None
        labels = [int(v) for v in labels]
        if len(labels) != k:
            raise ValueError(f"PrototypeBank: {len(labels)} labels for {k} classes")
        return labels

    def __len__(self):
        return int(self.protos.shape[0])

    def __repr__(self):
        return (f"PrototypeBank(K={len(self)}, p={self.p}, c={self.c}, {self.family}/{self.backbone}/{self.precision}, "
                f"dist_scalar={self.dist_scalar:g}, device={self.protos.device})")

    # -- persistence: plain tensors, ints, floats and strings -------------------------------------------------
    def state_dict(self):
        sd = {k: getattr(self, k) for k in _FIELDS}
        sd["protos"] = self.protos.detach().clone()
        sd["labels"] = None if self.labels is None else list(self.labels)
        return sd

    def load_state_dict(self, sd):
        """In place: the saved bank must have this bank's shape (``from_state_dict`` makes a new one)."""
        protos = sd["protos"]
        if tuple(protos.shape) != tuple(self.protos.shape):
            raise ValueError(f"PrototypeBank: saved protos {tuple(protos.shape)} do not fit this bank's {tuple(self.protos.shape)}")
        self.protos.copy_(protos)
        self.family, self.backbone, self.precision = str(sd["family"]), str(sd["backbone"]), str(sd["precision"])
        self.dist_scalar = float(sd["dist_scalar"])
        self.labels = self._labels(sd.get("labels"), len(self))
        return self

    @classmethod
    def from_state_dict(cls, sd, device=None):
        protos = sd["protos"].clone() if device is None else sd["protos"].to(device, copy=True)
        return cls(protos, sd["family"], sd["backbone"], sd["precision"], sd["dist_scalar"], sd.get("labels"))

    def to(self, device):
        """A bank on ``device`` (this one if it is there already)."""
        if self.protos.device == torch.device(device):
            return self
        return PrototypeBank(self.protos.to(device), self.family, self.backbone, self.precision, self.dist_scalar, self.labels)

    # -- in-place updates: a captured graph that reads ``protos`` sees them ------------------------------------
    def update(self, k, other, label=None):
        """Class ``k`` <- ``other``: a one-class bank made by the same kind of model, or a ``[2p, c]`` tensor.  Copies into the
        bank's own storage."""
        if not 0 <= int(k) < len(self):
            raise IndexError(f"PrototypeBank.update: class {k} of a bank of {len(self)}")
        if isinstance(other, PrototypeBank):
            self.require_like(other, "PrototypeBank.update")
            if len(other) != 1:
                raise ValueError(f"PrototypeBank.update: the source bank must hold one class, it holds {len(other)}")
            row = other.protos[0]
            if label is None and other.labels is not None:
                label = other.labels[0]
        else:
            row = other
        if tuple(row.shape) != (2 * self.p, self.c):
            raise ValueError(f"PrototypeBank.update: expected [{2 * self.p},{self.c}], got {tuple(row.shape)}")
        self.protos[int(k)].copy_(row)
        if label is not None:
            if self.labels is None:
                raise ValueError("PrototypeBank.update: this bank has no labels")
            self.labels[int(k)] = int(label)
        return self

    def require_like(self, other, what):
        """ValueError unless ``other`` was made by the same family / backbone / precision with the same p, c, dist_scalar."""
        for f in _FIELDS:
            if getattr(self, f) != getattr(other, f):
                raise ValueError(f"{what}: bank mismatch in {f}: {getattr(other, f)!r} against {getattr(self, f)!r}")
