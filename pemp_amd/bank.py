"""Prototype banks: the prototypes of K classes, enrolled once from their supports (``model.enroll``) and met by any
number of queries afterwards (``model.segment`` / ``segment_lowres`` / ``segment_graphed``).

The prototypes of the prototype-matching families -- PEMP stage 1 (meta-prototypes, or plain masked average pooling with
``protos = 0``), Baseline, PANet -- depend on the supports alone, so an episode's support passes through the trunk need not
be repeated for every query.  The bank keeps them in the layout the head kernels share (``[K, 2p, c]``, foreground rows
first) together with what a query pass must agree with: the model family, its backbone, the precision the trunk ran at,
``p``, ``c`` and ``dist_scalar``.

PFENet's head conditions on the query, its support side does not: ``PFENetBank`` keeps that side -- the packed support operand
of the prior GEMM and the support vectors -- with the same services; ``RPMMsBank`` keeps what RPMMs' support side ends in, the
prototypes of the mixture models and their products with ``layer55``.  All classes offer ``empty_like`` (an empty K-slot
sibling of a one-class bank), ``holds`` and ``tensors`` to the code that serves any of them
(``entry.pemp_stage1.BankEvaluator``, ``_HeadMixin.segment_graphed``)."""
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

    @classmethod
    def empty_like(cls, one, k, labels=None):
        """A bank of ``k`` empty (all-zero) slots that classes enrolled like ``one`` can be copied into (``update``)."""
        zeros = torch.zeros((int(k),) + tuple(one.protos.shape[1:]), dtype=torch.float32, device=one.protos.device)
        return cls(zeros, one.family, one.backbone, one.precision, one.dist_scalar, labels=labels)

    def holds(self, one):
        """Whether a class enrolled as ``one`` fits a slot of this bank."""
        return tuple(self.protos.shape[1:]) == tuple(one.protos.shape[1:])

    def tensors(self):
        """The device storage a captured graph reads."""
        return (self.protos,)

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


_PF_FIELDS = ("family", "backbone", "precision", "S", "HW", "C")


class PFENetBank:
    """PFENet's support bank.  The head conditions on the query, but everything the supports contribute to an episode depends
    on them alone: per (class, shot) the masked layer-4 rows of the prior GEMM with their norms (``ops.prior_bank_pack``: the
    foreground rows and one zero row, ``count`` of them in a slot of ``cap``), per class the Weighted-GAP support vector
    ``svec``.  ``count_host`` mirrors ``count`` on the host (capacity checks without a synchronisation)."""
    family = "pfenet"
    _labels = staticmethod(PrototypeBank._labels)

    def __init__(self, rows, norms, count, svec, hw, backbone, precision, labels=None, count_host=None):
        if rows.dim() != 4 or rows.dtype != torch.float32 or min(rows.shape) < 1 or rows.shape[2] % 64 or rows.shape[3] % 32:
            raise ValueError(f"PFENetBank: rows must be fp32 [K,S,cap,C] with cap % 64 == 0 and C % 32 == 0, got "
                             f"{tuple(rows.shape)} {rows.dtype}")
        K, S, cap, C = (int(v) for v in rows.shape)
        if tuple(norms.shape) != (K, S, cap) or norms.dtype != torch.float32:
            raise ValueError(f"PFENetBank: norms must be fp32 [{K},{S},{cap}], got {tuple(norms.shape)} {norms.dtype}")
        if tuple(count.shape) != (K, S) or count.dtype != torch.int32:
            raise ValueError(f"PFENetBank: count must be int32 [{K},{S}], got {tuple(count.shape)} {count.dtype}")
        if svec.dim() != 2 or svec.shape[0] != K or svec.dtype != torch.float32:
            raise ValueError(f"PFENetBank: svec must be fp32 [{K},c], got {tuple(svec.shape)} {svec.dtype}")
        if any(t.device != rows.device for t in (norms, count, svec)):
            raise ValueError("PFENetBank: rows, norms, count and svec must lie on one device")
        self.rows, self.norms, self.count, self.svec = rows.contiguous(), norms.contiguous(), count.contiguous(), svec.contiguous()
        self.count_host = (self.count.cpu() if count_host is None else count_host.to("cpu", torch.int32)).clone()
        self.S, self.cap, self.C, self.HW = S, cap, C, int(hw)
        if tuple(self.count_host.shape) != (K, S) or int(self.count_host.min()) < 1 or int(self.count_host.max()) > min(cap, self.HW):
            raise ValueError(f"PFENetBank: every count must lie in 1..min(cap, HW) = {min(cap, self.HW)}, got "
                             f"{self.count_host.tolist()}")
        self.backbone, self.precision = str(backbone), str(precision)
        self.labels = self._labels(labels, K)

    def __len__(self):
        return int(self.rows.shape[0])

    def __repr__(self):
        return (f"PFENetBank(K={len(self)}, S={self.S}, HW={self.HW}, C={self.C}, cap={self.cap}, "
                f"{self.family}/{self.backbone}/{self.precision}, device={self.rows.device})")

    def nbytes(self):
        """Bytes of device storage per class."""
        return sum(t.numel() * t.element_size() for t in self.tensors()) // len(self)

    def tensors(self):
        """The device storage a captured graph reads."""
        return (self.rows, self.norms, self.count, self.svec)

    @classmethod
    def empty_like(cls, one, k, labels=None, cap=None):
        """A bank of ``k`` empty slots (one zero row each: the prior of an empty mask) for classes enrolled like ``one``;
        ``cap`` defaults to HW rounded up to 64, which holds any mask."""
        cap = -(-one.HW // 64) * 64 if cap is None else int(cap)
        dev, k = one.rows.device, int(k)
        return cls(torch.zeros((k, one.S, cap, one.C), dtype=torch.float32, device=dev),
                   torch.zeros((k, one.S, cap), dtype=torch.float32, device=dev),
                   torch.ones((k, one.S), dtype=torch.int32, device=dev),
                   torch.zeros((k, one.svec.shape[1]), dtype=torch.float32, device=dev), one.HW, one.backbone, one.precision,
                   labels=labels, count_host=torch.ones((k, one.S), dtype=torch.int32))

    def holds(self, one):
        """Whether a class enrolled as ``one`` fits a slot of this bank."""
        return all(getattr(self, f) == getattr(one, f) for f in ("S", "HW", "C")) and self.svec.shape[1] == one.svec.shape[1] \
            and int(one.count_host.max()) <= self.cap

    # -- persistence: plain tensors, ints and strings -------------------------------------------------------------
    def state_dict(self):
        sd = {k: getattr(self, k) for k in _PF_FIELDS}
        for k in ("rows", "norms", "count", "svec"):
            sd[k] = getattr(self, k).detach().clone()
        sd["labels"] = None if self.labels is None else list(self.labels)
        return sd

    @classmethod
    def from_state_dict(cls, sd, device=None):
        if sd.get("family") != cls.family:
            raise ValueError(f"PFENetBank: the saved bank's family is {sd.get('family')!r}")
        mv = (lambda t: t.clone()) if device is None else (lambda t: t.to(device, copy=True))
        return cls(mv(sd["rows"]), mv(sd["norms"]), mv(sd["count"]), mv(sd["svec"]), sd["HW"], sd["backbone"], sd["precision"],
                   sd.get("labels"), count_host=sd["count"])

    def load_state_dict(self, sd):
        """In place: the saved bank must have this bank's shape (``from_state_dict`` makes a new one)."""
        if tuple(sd["rows"].shape) != tuple(self.rows.shape) or int(sd["HW"]) != self.HW or sd.get("family") != self.family:
            raise ValueError(f"PFENetBank: saved rows {tuple(sd['rows'].shape)} (HW = {sd['HW']}) do not fit this bank's "
                             f"{tuple(self.rows.shape)} (HW = {self.HW})")
        for k in ("rows", "norms", "count", "svec"):
            getattr(self, k).copy_(sd[k])
        self.count_host.copy_(sd["count"])
        self.backbone, self.precision = str(sd["backbone"]), str(sd["precision"])
        self.labels = self._labels(sd.get("labels"), len(self))
        return self

    def to(self, device):
        """A bank on ``device`` (this one if it is there already)."""
        if self.rows.device == torch.device(device):
            return self
        return PFENetBank(self.rows.to(device), self.norms.to(device), self.count.to(device), self.svec.to(device), self.HW,
                          self.backbone, self.precision, self.labels, count_host=self.count_host)

    # -- in-place updates: a captured graph that reads the bank sees them -------------------------------------------
    def update(self, k, other, label=None):
        """Class ``k`` <- ``other``, a one-class bank made by the same kind of model at the same input size (its ``cap`` may
        differ: what counts is that its rows fit).  Copies into the bank's own storage."""
        if not 0 <= int(k) < len(self):
            raise IndexError(f"PFENetBank.update: class {k} of a bank of {len(self)}")
        if not isinstance(other, PFENetBank):
            raise TypeError(f"PFENetBank.update: expected a PFENetBank, got {type(other).__name__}")
        self.require_like(other, "PFENetBank.update")
        if len(other) != 1:
            raise ValueError(f"PFENetBank.update: the source bank must hold one class, it holds {len(other)}")
        need = int(other.count_host.max())
        if need > self.cap:
            raise ValueError(f"PFENetBank.update: the class needs {need} rows, this bank's cap is {self.cap}")
        k, n = int(k), min(self.cap, other.cap)
        self.rows[k, :, :n].copy_(other.rows[0, :, :n])
        self.norms[k, :, :n].copy_(other.norms[0, :, :n])
        self.count[k].copy_(other.count[0])
        self.count_host[k] = other.count_host[0]
        self.svec[k].copy_(other.svec[0])
        if label is None and other.labels is not None:
            label = other.labels[0]
        if label is not None:
            if self.labels is None:
                raise ValueError("PFENetBank.update: this bank has no labels")
            self.labels[k] = int(label)
        return self

    def require_like(self, other, what):
        """ValueError unless ``other`` was made by the same backbone / precision with the same S, HW and C."""
        for f in _PF_FIELDS:
            if getattr(self, f) != getattr(other, f):
                raise ValueError(f"{what}: bank mismatch in {f}: {getattr(other, f)!r} against {getattr(self, f)!r}")


_RP_FIELDS = ("family", "backbone", "precision", "C")
_RP_COLS = 10          # ops.RPMMS_COLS: the three mixtures K = 1 | 3 | 6 side by side


class RPMMsBank:
    """RPMMs' support bank.  Everything an episode's support contributes -- its trunk pass, ``layer5``, the mask resize and the
    ten-iteration PMMs EM -- ends in ``mu`` [K,2,10,C] (side 0: foreground, 1: background; ``ops.rpmms_em``); ``taps`` [K,10,9,C]
    are the products of the foreground prototypes with the prototype half of ``layer55`` (``ops.rpmms_proto_taps``).  112 KB per
    class at C = 256.

    ``mu`` and ``taps`` belong to the weights and to the ``pmm_mu0`` that were current at enrolment: a model whose weights
    change, or whose initial mu is redrawn, does not change an enrolled bank.  The bank holds nothing that depends on the image
    size: queries of any size the trunk takes may meet it, whatever size its supports had."""
    family = "rpmms"
    _labels = staticmethod(PrototypeBank._labels)

    def __init__(self, mu, taps, backbone, precision, labels=None):
        if mu.dim() != 4 or mu.dtype != torch.float32 or mu.shape[0] < 1 or tuple(mu.shape[1:3]) != (2, _RP_COLS) or mu.shape[3] < 1:
            raise ValueError(f"RPMMsBank: mu must be fp32 [K,2,{_RP_COLS},C], got {tuple(mu.shape)} {mu.dtype}")
        K, C = int(mu.shape[0]), int(mu.shape[3])
        if tuple(taps.shape) != (K, _RP_COLS, 9, C) or taps.dtype != torch.float32:
            raise ValueError(f"RPMMsBank: taps must be fp32 [{K},{_RP_COLS},9,{C}], got {tuple(taps.shape)} {taps.dtype}")
        if taps.device != mu.device:
            raise ValueError("RPMMsBank: mu and taps must lie on one device")
        self.mu, self.taps = mu.contiguous(), taps.contiguous()
        self.C = C
        self.backbone, self.precision = str(backbone), str(precision)
        self.labels = self._labels(labels, K)

    def __len__(self):
        return int(self.mu.shape[0])

    def __repr__(self):
        return f"RPMMsBank(K={len(self)}, C={self.C}, {self.family}/{self.backbone}/{self.precision}, device={self.mu.device})"

    def nbytes(self):
        """Bytes of device storage per class."""
        return sum(t.numel() * t.element_size() for t in self.tensors()) // len(self)

    def tensors(self):
        """The device storage a captured graph reads."""
        return (self.mu, self.taps)

    @classmethod
    def empty_like(cls, one, k, labels=None):
        """A bank of ``k`` empty (all-zero) slots for classes enrolled like ``one``."""
        dev, k = one.mu.device, int(k)
        return cls(torch.zeros((k, 2, _RP_COLS, one.C), dtype=torch.float32, device=dev),
                   torch.zeros((k, _RP_COLS, 9, one.C), dtype=torch.float32, device=dev), one.backbone, one.precision, labels=labels)

    def holds(self, one):
        """Whether a class enrolled as ``one`` fits a slot of this bank."""
        return isinstance(one, RPMMsBank) and self.C == one.C

    # -- persistence: plain tensors, ints and strings -------------------------------------------------------------
    def state_dict(self):
        sd = {k: getattr(self, k) for k in _RP_FIELDS}
        sd["mu"], sd["taps"] = self.mu.detach().clone(), self.taps.detach().clone()
        sd["labels"] = None if self.labels is None else list(self.labels)
        return sd

    @classmethod
    def from_state_dict(cls, sd, device=None):
        if sd.get("family") != cls.family:
            raise ValueError(f"RPMMsBank: the saved bank's family is {sd.get('family')!r}")
        mv = (lambda t: t.clone()) if device is None else (lambda t: t.to(device, copy=True))
        return cls(mv(sd["mu"]), mv(sd["taps"]), sd["backbone"], sd["precision"], sd.get("labels"))

    def load_state_dict(self, sd):
        """In place: the saved bank must have this bank's shape (``from_state_dict`` makes a new one)."""
        if tuple(sd["mu"].shape) != tuple(self.mu.shape) or tuple(sd["taps"].shape) != tuple(self.taps.shape) \
                or sd.get("family") != self.family:
            raise ValueError(f"RPMMsBank: saved mu {tuple(sd['mu'].shape)} ({sd.get('family')!r}) does not fit this bank's "
                             f"{tuple(self.mu.shape)}")
        self.mu.copy_(sd["mu"])
        self.taps.copy_(sd["taps"])
        self.backbone, self.precision = str(sd["backbone"]), str(sd["precision"])
        self.labels = self._labels(sd.get("labels"), len(self))
        return self

    def to(self, device):
        """A bank on ``device`` (this one if it is there already)."""
        if self.mu.device == torch.device(device):
            return self
        return RPMMsBank(self.mu.to(device), self.taps.to(device), self.backbone, self.precision, self.labels)

    # -- in-place updates: a captured graph that reads the bank sees them -------------------------------------------
    def update(self, k, other, label=None):
        """Class ``k`` <- ``other``, a one-class bank made by the same kind of model.  Copies into the bank's own storage."""
        if not 0 <= int(k) < len(self):
            raise IndexError(f"RPMMsBank.update: class {k} of a bank of {len(self)}")
        if not isinstance(other, RPMMsBank):
            raise TypeError(f"RPMMsBank.update: expected an RPMMsBank, got {type(other).__name__}")
        self.require_like(other, "RPMMsBank.update")
        if len(other) != 1:
            raise ValueError(f"RPMMsBank.update: the source bank must hold one class, it holds {len(other)}")
        k = int(k)
        self.mu[k].copy_(other.mu[0])
        self.taps[k].copy_(other.taps[0])
        if label is None and other.labels is not None:
            label = other.labels[0]
        if label is not None:
            if self.labels is None:
                raise ValueError("RPMMsBank.update: this bank has no labels")
            self.labels[k] = int(label)
        return self

    def require_like(self, other, what):
        """ValueError unless ``other`` was made by the same backbone / precision with the same C."""
        for f in _RP_FIELDS:
            if getattr(self, f) != getattr(other, f):
                raise ValueError(f"{what}: bank mismatch in {f}: {getattr(other, f)!r} against {getattr(self, f)!r}")
