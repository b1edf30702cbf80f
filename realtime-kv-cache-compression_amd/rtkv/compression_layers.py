"""CompressedKVCache and AdaptiveQuantization — the compression_layers API surface named by the
north_star (reference src/models/compression_layers.py:7-45 and :96-175).

CompressedKVCache keeps the reference's dict-of-tensors interface and adds the packed form of a layer
(bit-packed integer codes + per-row scale/zero-point, as produced by rtkv_compress_layer) with an
on-device decoder (rtkv_unpack_dequant) that reproduces the dequantized K'/V' bit for bit.

Generation: the reference's decode steps do not compress; each appends the new token's dense K/V to
the cache and attends over everything (modified_llama.py:83-94, 152).  DecodeTail holds those dense
rows of one layer, and decode_attention(..., tail=...) attends over the packed rows followed by them
(rtkv_decode_attention_packed_tail) without dequantizing the layer.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Optional

import torch
import torch.nn as nn

from . import _lib as L
from .token_importance import _workspace


class CompressedKVCache:
    """Per-layer storage of compressed K/V (compression_layers.py:7-45)."""

    def __init__(self, max_batch_size: int, max_seq_len: int, head_dim: int, tail_capacity: int = 256):
        self.max_batch_size = max_batch_size
        self.max_seq_len = max_seq_len
        self.head_dim = head_dim
        self.tail_capacity = tail_capacity  # first allocation of a layer's DecodeTail (it doubles when full)
        self.cache_data: Dict[int, dict] = {}
        self.compression_info: Dict[int, dict] = {}
        self.tails: Dict[int, "DecodeTail"] = {}
        self.gq: Dict[int, "GroupQuantKVCache"] = {}  # layers served from the rtkv-gq/1 format

    def store_compressed_kv(self, layer_idx: int, keys: torch.Tensor, values: torch.Tensor,
                            importance_scores: torch.Tensor, precision_labels: torch.Tensor,
                            selection_mask: torch.Tensor):
        self.cache_data[layer_idx] = {
            "keys": keys.detach(),
            "values": values.detach(),
            "importance_scores": importance_scores.detach(),
            "precision_labels": precision_labels.detach(),
            "selection_mask": selection_mask.detach(),
            "compressed_seq_len": keys.shape[1],
        }

    def get_compressed_kv(self, layer_idx: int) -> Optional[Dict]:
        return self.cache_data.get(layer_idx)

    def clear_cache(self):
        self.cache_data.clear()
        self.compression_info.clear()
        self.tails.clear()
        self.gq.clear()

    # ------------------------------------------------------------------ packed form (extension)
    def store_packed(self, layer_idx: int, packed: dict):
        """Keep only the packed codes of a layer (``info['packed']`` of compress_layer_kv_cache)."""
        self.compression_info[layer_idx] = packed
        self.gq.pop(layer_idx, None)
        self.tails.pop(layer_idx, None)  # a new prefill: the tokens generated after the old one are gone

    def store_group_quant(self, layer_idx: int, cache: "GroupQuantKVCache"):
        """Serve a layer from the rtkv-gq/1 format (``info['group_quant']`` of compress_layer_kv_cache with
        ``group_quant=``): append, tail_len, attend and attend_chunk then work on it as on a packed layer,
        so CompressedDecodeAttention generates over it unchanged.  The format has no file form: save,
        load, packed_nbytes and dequantize refuse such a layer (use cache.nbytes() / cache.dequantize())."""
        from .group_quant import GroupQuantKVCache
        if not isinstance(cache, GroupQuantKVCache):
            raise ValueError("store_group_quant takes a GroupQuantKVCache (info['group_quant'])")
        self.gq[layer_idx] = cache
        self.compression_info.pop(layer_idx, None)
        self.tails.pop(layer_idx, None)  # a new prefill: the tokens generated after the old one are gone

    def _no_gq(self, layer_idx, what: str):
        if layer_idx in self.gq:
            raise ValueError(f"{what}: layer {layer_idx} is held in the rtkv-gq/1 format, which has no per-token "
                             f"packed form and no file format (use the GroupQuantKVCache's own methods)")

    def packed_nbytes(self, layer_idx: int) -> int:
        self._no_gq(layer_idx, "packed_nbytes")
        p = self.compression_info[layer_idx]
        return (p["codes_k"].numel() + p["codes_v"].numel() + p["scale_zp"].numel() * 4
                + p["kept_index"].numel() * 4)

    def dequantize(self, layer_idx: int):
        """Decode a packed layer back to dense (K', V') [B, S'_max, F] on the device."""
        self._no_gq(layer_idx, "dequantize")
        p = self.compression_info[layer_idx]
        return unpack_layer(p)

    def attend(self, layer_idx: int, q: torch.Tensor, num_kv_heads: int, scale: Optional[float] = None):
        """One decode step of attention over the packed layer (no dense K'/V'), followed by the
        layer's appended tokens when there are any: fp32 [B, Hq, D]."""
        g = self.gq.get(layer_idx)
        if g is not None:
            _gq_heads(g, q, num_kv_heads)
            return g.attend(q, scale, tail=self.tails.get(layer_idx))
        return decode_attention(self.compression_info[layer_idx], q, num_kv_heads, scale,
                                tail=self.tails.get(layer_idx))

    def attend_chunk(self, layer_idx: int, q: torch.Tensor, num_kv_heads: int, scale: Optional[float] = None):
        """Attention of the T newest tokens (q [B, Hq, T, D]; their K/V are already the last T rows of
        the layer's tail) over the packed layer and the tail, causal among the new tokens: fp32
        [B, Hq, T, D] (extend_attention)."""
        t = self.tails.get(layer_idx)
        if t is None:
            raise ValueError(f"layer {layer_idx} has no appended tokens: append the chunk's K/V first")
        g = self.gq.get(layer_idx)
        if g is not None:
            return gq_extend_attention(g, q, num_kv_heads, t, scale)
        return extend_attention(self.compression_info[layer_idx], q, num_kv_heads, t, scale)

    def append(self, layer_idx: int, k_new: torch.Tensor, v_new: torch.Tensor):
        """Append the dense K/V of newly generated tokens ([B, F] or [B, T, F], the layout
        compress_layer_kv_cache takes) behind the layer's packed rows (modified_llama.py:83-94: a
        decode step concatenates, it does not compress).  The layer's DecodeTail is created on first
        use with the packed layer's dtype, feature_dim and batch size."""
        t = self.tails.get(layer_idx)
        if t is None and layer_idx in self.gq:
            g = self.gq[layer_idx]
            t = self.tails[layer_idx] = DecodeTail(1, g.F, g.dtype, g.device, capacity=self.tail_capacity)
        elif t is None:
            p = self.compression_info[layer_idx]
            t = self.tails[layer_idx] = DecodeTail(p["kept_index"].shape[0], int(p["feature_dim"]), p["dtype"],
                                                   p["codes_k"].device, capacity=self.tail_capacity)
        t.append(k_new, v_new)

    def tail_len(self, layer_idx: int) -> int:
        """Tokens appended to the layer since its packed rows were stored."""
        t = self.tails.get(layer_idx)
        return 0 if t is None else len(t)

    def save(self, path: str):
        """Write every packed layer to one safetensors file (see save_packed for the format).
        Appended tokens (the DecodeTails) are not serialized: the file holds the prefill only."""
        for i in self.gq:
            self._no_gq(i, "save")
        save_packed(self.compression_info, path)

    def load(self, path: str, device="cuda"):
        """Read the packed layers of a file written by save(); replaces the packed layers held and
        drops every tail (the file has none)."""
        for i in self.gq:
            self._no_gq(i, "load")
        self.compression_info = load_packed(path, device)
        self.tails.clear()


class DecodeTail:
    """The dense K/V rows of the tokens generated after the prefill, for one layer: k, v
    [B, capacity, F] in the K/V dtype and rows_dev (int64 [B], rows in use), all on one device.
    append() copies with torch ops and advances rows_dev on the device — no host→device copy per
    step — and doubles the buffers when they are full.  Not serialized with the packed layers."""

    def __init__(self, B: int, feature_dim: int, dtype: torch.dtype, device, capacity: int = 256):
        if dtype not in L.TORCH_DTYPE_CODE:
            raise ValueError(f"DecodeTail: unsupported dtype {dtype} (float32, float16, bfloat16)")
        if B < 1 or feature_dim < 1 or capacity < 1:
            raise ValueError("DecodeTail: B, feature_dim and capacity must be positive")
        if (feature_dim * torch.empty(0, dtype=dtype).element_size()) % 16:
            raise ValueError("DecodeTail: rows must be a multiple of 16 bytes")
        self.k = torch.zeros(B, capacity, feature_dim, dtype=dtype, device=device)
        self.v = torch.zeros_like(self.k)
        self.rows_dev = torch.zeros(B, dtype=torch.int64, device=device)
        self._len: Optional[int] = 0  # rows appended (the same for every batch row); None: caller-owned

    @classmethod
    def from_tensors(cls, k: torch.Tensor, v: torch.Tensor, rows: torch.Tensor) -> "DecodeTail":
        """Wrap caller-owned buffers k, v [B, capacity, F] (same dtype, device and strides, unit
        stride along F, batch and row strides and the base 16-byte aligned) with per-row counts
        `rows` (int64 [B]) that may differ.  Counts are checked against [0, capacity] when `rows`
        is on the host (it is then copied to the buffers' device once); on the device the kernel
        clamps them.  Such a tail cannot be appended to."""
        if k.dim() != 3 or v.shape != k.shape:
            raise ValueError("DecodeTail: k and v must both be [B, capacity, F]")
        if k.dtype not in L.TORCH_DTYPE_CODE or v.dtype != k.dtype:
            raise ValueError(f"DecodeTail: k and v must share one of float32/float16/bfloat16 (got {k.dtype}, {v.dtype})")
        if v.device != k.device:
            raise ValueError("DecodeTail: k and v are on different devices")
        B, cap, F = k.shape
        if rows.dtype != torch.int64 or rows.shape != (B,):
            raise ValueError(f"DecodeTail: rows must be int64 [{B}], got {rows.dtype} {tuple(rows.shape)}")
        e = k.element_size()
        if cap > 0 and B * F > 0:
            if k.stride() != v.stride() or k.stride(2) != 1 or k.stride(1) < F:
                raise ValueError("DecodeTail: k and v need the same strides, unit stride along F and stride_s >= F")
            if (k.stride(0) * e) % 16 or (k.stride(1) * e) % 16 or k.data_ptr() % 16 or v.data_ptr() % 16:
                raise ValueError("DecodeTail: base pointers, stride_b and stride_s must keep rows 16-byte aligned")
        if not rows.is_cuda:
            if any(int(r) < 0 or int(r) > cap for r in rows.tolist()):
                raise ValueError(f"DecodeTail: row counts {rows.tolist()} outside [0, {cap}]")
            rows = rows.to(k.device)
        elif rows.device != k.device:
            raise ValueError("DecodeTail: rows is on another device than k and v")
        t = cls.__new__(cls)
        t.k, t.v, t.rows_dev, t._len = k, v, rows.contiguous(), None
        return t

    @property
    def capacity(self) -> int:
        return self.k.shape[1]

    def __len__(self) -> int:
        if self._len is None:
            raise TypeError("DecodeTail.from_tensors: the row counts live in rows_dev")
        return self._len

    def append(self, k_new: torch.Tensor, v_new: torch.Tensor):
        """k_new, v_new: [B, F] or [B, T, F] (T >= 1), the layout compress_layer_kv_cache takes."""
        if self._len is None:
            raise ValueError("DecodeTail.from_tensors wraps caller-owned buffers: append to them directly")
        if k_new.dim() == 2:
            k_new, v_new = k_new.unsqueeze(1), v_new.unsqueeze(1) if v_new.dim() == 2 else v_new
        B, cap, F = self.k.shape
        if k_new.dim() != 3 or v_new.shape != k_new.shape or k_new.shape[0] != B or k_new.shape[2] != F \
                or k_new.shape[1] < 1:
            raise ValueError(f"DecodeTail.append: expected [{B}, {F}] or [{B}, T, {F}], got {tuple(k_new.shape)} / "
                             f"{tuple(v_new.shape)}")
        if k_new.dtype != self.k.dtype or v_new.dtype != self.k.dtype:
            raise ValueError(f"DecodeTail.append: dtype {k_new.dtype} / {v_new.dtype}, the tail holds {self.k.dtype}")
        if k_new.device != self.k.device or v_new.device != self.k.device:
            raise ValueError(f"DecodeTail.append: tensors on {k_new.device}, the tail is on {self.k.device}")
        T, n = k_new.shape[1], self._len
        if n + T > cap:
            while cap < n + T:
                cap *= 2
            for name in ("k", "v"):
                old = getattr(self, name)
                new = torch.zeros(B, cap, F, dtype=old.dtype, device=old.device)
                new[:, :n] = old[:, :n]
                setattr(self, name, new)
        self.k[:, n:n + T] = k_new
        self.v[:, n:n + T] = v_new
        self.rows_dev += T
        self._len = n + T


# ---------------------------------------------------------------------- packed (de)serialization
# File format "rtkv-packed/1": a safetensors file.  Per layer i, tensors "L{i}.codes_k",
# "L{i}.codes_v" (uint8, the bit-packed rows back to back), "L{i}.row_offset" (int64 [B, S'] byte
# offset of each kept row), "L{i}.scale_zp" (fp32 [B, S', 4]: K scale, K zero-point, V scale,
# V zero-point), "L{i}.kept_index" (int32 [B, S'] source token index), "L{i}.labels" (uint8 [B, S]
# precision class per source token); the metadata entry "L{i}" holds {"rows", "bits", "dtype",
# "feature_dim"} as JSON.  Loading checks every offset and count against the tensor sizes, so a
# truncated or inconsistent file raises ValueError instead of reaching a kernel.
_FORMAT = "rtkv-packed/1"
_TENSORS = ("codes_k", "codes_v", "row_offset", "scale_zp", "kept_index", "labels")
_DTYPES = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}


def save_packed(layers: Dict[int, dict], path: str):
    import json
    from safetensors.torch import save_file
    tensors, meta = {}, {"format": _FORMAT}
    for i, p in layers.items():
        for name in _TENSORS:
            tensors[f"L{i}.{name}"] = p[name].detach().contiguous().cpu()
        meta[f"L{i}"] = json.dumps({"rows": [int(r) for r in p["rows"]], "bits": [int(b) for b in p["bits"]],
                                    "dtype": str(p["dtype"]).replace("torch.", ""),
                                    "feature_dim": int(p["feature_dim"])})
    save_file(tensors, path, metadata=meta)


_TENSOR_DTYPES = {"codes_k": torch.uint8, "codes_v": torch.uint8, "row_offset": torch.int64,
                  "scale_zp": torch.float32, "kept_index": torch.int32, "labels": torch.uint8}


def _check_dtypes(where, p: dict):
    """The kernels read these buffers with fixed element types; a wrong dtype would be misread or
    read past its end."""
    for name, dt in _TENSOR_DTYPES.items():
        if p[name].dtype != dt:
            raise ValueError(f"packed layer {where}: {name} must be {dt}, got {p[name].dtype}")


def _check_packed(i: int, p: dict):
    def bad(msg):
        raise ValueError(f"packed layer {i}: {msg}")
    _check_dtypes(i, p)
    if p["kept_index"].dim() != 2:
        bad("kept_index must be [B, S']")
    B, Sp = p["kept_index"].shape
    if p["row_offset"].shape != (B, Sp) or p["scale_zp"].shape != (B, Sp, 4) or p["labels"].dim() != 2 \
            or p["labels"].shape[0] != B:
        bad("inconsistent shapes")
    if p["codes_k"].numel() != p["codes_v"].numel():
        bad("codes_k and codes_v differ in size")
    if len(p["rows"]) != B or any(r < 0 or r > Sp for r in p["rows"]):
        bad("row counts out of range")
    F, S = p["feature_dim"], p["labels"].shape[1]
    widths = [L.lib().rtkv_field_width(L.TORCH_DTYPE_CODE[p["dtype"]], b) for b in p["bits"]]
    if len(widths) != 3 or min(widths) <= 0:
        bad("unsupported bits")
    nbytes = p["codes_k"].numel()
    for b in range(B):
        n = p["rows"][b]
        if n == 0:
            continue
        ki = p["kept_index"][b, :n].to(torch.int64)
        if int(ki.min()) < 0 or int(ki.max()) >= S:
            bad("kept index out of range")
        lab = p["labels"][b].to(torch.int64)[ki]
        if int(lab.max()) > 2:
            bad("class label out of range")
        w = torch.tensor(widths, dtype=torch.int64)[lab]
        off = p["row_offset"][b, :n]
        if int(off.min()) < 0 or int((off + F * w // 8).max()) > nbytes:
            bad("row offsets past the end of the codes")


def load_packed(path: str, device="cuda") -> Dict[int, dict]:
    import json
    from safetensors import safe_open
    out: Dict[int, dict] = {}
    with safe_open(path, framework="pt", device="cpu") as f:
        meta = f.metadata() or {}
        if meta.get("format") != _FORMAT:
            raise ValueError(f"{path}: not an {_FORMAT} file")
        for key, val in meta.items():
            if not key.startswith("L"):
                continue
            i = int(key[1:])
            m = json.loads(val)
            p = {name: f.get_tensor(f"L{i}.{name}") for name in _TENSORS}
            if m["dtype"] not in _DTYPES:
                raise ValueError(f"packed layer {i}: unknown dtype {m['dtype']}")
            p.update(rows=list(m["rows"]), bits=tuple(m["bits"]), dtype=_DTYPES[m["dtype"]],
                     feature_dim=int(m["feature_dim"]))
            _check_packed(i, p)
            for name in _TENSORS:
                p[name] = p[name].to(device)
            out[i] = p
    return dict(sorted(out.items()))


def unpack_layer(p: dict):
    """Packed layer dict → dense dequantized (K', V'), bit-identical to the fused output."""
    codes_k, codes_v = p["codes_k"], p["codes_v"]
    L.require_device(codes_k, codes_v)
    dev = codes_k.device
    row_offset = p["row_offset"].contiguous()
    scale_zp = p["scale_zp"].contiguous()
    kept_index = p["kept_index"].contiguous()
    labels = p["labels"].contiguous()
    B, Sp = kept_index.shape
    S = labels.shape[1]
    F = int(p["feature_dim"])
    dtype = p["dtype"]
    rows = torch.tensor(p["rows"], dtype=torch.int64, device=dev)
    bits = (ctypes.c_int32 * 3)(*p["bits"])
    outs = []
    for which, codes in ((0, codes_k), (1, codes_v)):
        out = torch.zeros(B, Sp, F, dtype=dtype, device=dev)
        if out.numel():
            L.check(L.lib().rtkv_unpack_dequant(codes.data_ptr(), row_offset.data_ptr(), scale_zp.data_ptr(), which,
                                                kept_index.data_ptr(), labels.data_ptr(), B, S, Sp, rows.data_ptr(), 1,
                                                F, L.TORCH_DTYPE_CODE[dtype], bits, out.data_ptr(), Sp * F, F, F,
                                                L.stream_ptr(dev)), "rtkv_unpack_dequant")
        outs.append(out)
    return outs[0], outs[1]


def _packed_args(where: str, p: dict, q: torch.Tensor, B: int, D: int, num_kv_heads: int, dev, nullable: bool):
    """The packed layer dict `p` checked against a query (q's dtype, B batch rows, num_kv_heads heads of
    D) and marshalled as the 15 leading arguments of the attention entry points.  Returns (args, Sp,
    keep): Sp the layer's row capacity, keep the tensors the pointers belong to (the caller holds it across the
    call).  nullable: a layer without row capacity passes null pointers (the tail forms)."""
    if q.dtype != p["dtype"]:
        raise ValueError(f"q dtype {q.dtype} does not match the packed layer's {p['dtype']}")
    F = int(p["feature_dim"])
    if num_kv_heads * D != F:
        raise ValueError(f"num_kv_heads * head_dim = {num_kv_heads * D} != feature_dim {F}")
    codes_k, codes_v = p["codes_k"], p["codes_v"]
    row_offset = p["row_offset"].contiguous()
    scale_zp = p["scale_zp"].contiguous()
    kept_index = p["kept_index"].contiguous()
    labels = p["labels"].contiguous()
    _check_dtypes(where, p)
    # the kernels index every per-batch array by q's batch row: they must all have B rows
    if kept_index.dim() != 2 or kept_index.shape[0] != B or len(p["rows"]) != B or labels.shape[0] != B \
            or row_offset.shape[0] != B or scale_zp.shape[0] != B:
        raise ValueError(f"q has {B} batch rows but the packed layer has {kept_index.shape[0]} "
                         f"(rows {len(p['rows'])}, labels {labels.shape[0]})")
    Sp = kept_index.shape[1]
    if row_offset.shape != (B, Sp) or scale_zp.shape != (B, Sp, 4):
        raise ValueError("packed layer: row_offset / scale_zp shapes disagree with kept_index")
    if codes_k.numel() != codes_v.numel():
        raise ValueError("codes_k and codes_v differ in size")
    if any(int(r) < 0 or int(r) > Sp for r in p["rows"]):
        raise ValueError(f"row counts {p['rows']} outside [0, {Sp}]")
    rows = p.get("_rows_dev")
    if rows is None or rows.device != dev:  # kept once per layer: no host→device copy per decode step
        rows = p["_rows_dev"] = torch.tensor(p["rows"], dtype=torch.int64, device=dev)
    keep = (codes_k, codes_v, row_offset, scale_zp, kept_index, labels, rows)
    pk = (lambda t: 0) if nullable and Sp == 0 else (lambda t: t.data_ptr())
    args = (pk(codes_k), pk(codes_v), codes_k.numel(), pk(row_offset), pk(scale_zp), pk(kept_index), pk(labels), B,
            labels.shape[1], Sp, pk(rows), num_kv_heads, D, L.TORCH_DTYPE_CODE[q.dtype], (ctypes.c_int32 * 3)(*p["bits"]))
    return args, Sp, keep


def _dense_tail(tail: "DecodeTail", q: torch.Tensor, B: int, F: int) -> "L.DenseTail":
    """rtkv_dense_tail of `tail`, checked against q's batch, dtype and device and the feature_dim."""
    if tail.k.dtype != q.dtype or tail.k.shape[0] != B or tail.k.shape[2] != F or tail.k.device != q.device \
            or tail.v.shape != tail.k.shape or tail.rows_dev.shape != (B,) or tail.rows_dev.dtype != torch.int64:
        raise ValueError(f"tail [{tuple(tail.k.shape)} {tail.k.dtype}] does not match q's batch {B}, feature_dim {F}, "
                         f"dtype {q.dtype}")
    cap = tail.capacity
    return L.DenseTail(L.ptr(tail.k) if cap else 0, L.ptr(tail.v) if cap else 0, tail.rows_dev.data_ptr(), cap,
                       tail.k.stride(0), tail.k.stride(1))


def decode_attention(p: dict, q: torch.Tensor, num_kv_heads: int, scale: Optional[float] = None,
                     tail: Optional[DecodeTail] = None) -> torch.Tensor:
    """Attention of one new token per batch row over a packed layer, decoded on the fly
    (rtkv_decode_attention_packed).  q: [B, Hq, D] in the layer's dtype; returns fp32 [B, Hq, D] =
    softmax(q·K'ᵀ·scale)·V' over the kept rows, with K'/V' exactly the dequantized rows
    (modified_llama.py:140-142 attends over those dequantized floats).  scale defaults to 1/sqrt(D)
    (modified_llama.py:89).  tail: the dense rows of the tokens generated since (DecodeTail); the
    softmax then runs over the kept rows followed by the tail's rows, what a decode step of the
    reference attends over (modified_llama.py:83-94, 152; rtkv_decode_attention_packed_tail)."""
    if tail is not None:
        return _decode_attention_tail(p, q, num_kv_heads, scale, tail)
    L.require_device(p["codes_k"], p["codes_v"], q)
    dev = p["codes_k"].device
    B, Hq, D = q.shape
    args, Sp, _keep = _packed_args("decode", p, q, B, D, num_kv_heads, dev, nullable=False)
    out = torch.zeros(B, Hq, D, dtype=torch.float32, device=dev)
    if Sp == 0:
        return out
    qc = q.contiguous()
    ws = torch.empty(L.lib().rtkv_decode_workspace_size(B, Hq, num_kv_heads, D, Sp), dtype=torch.uint8, device=dev)
    sc = float(scale) if scale is not None else 1.0 / float(D) ** 0.5
    L.check(L.lib().rtkv_decode_attention_packed(*args, qc.data_ptr(), Hq, sc, out.data_ptr(), ws.data_ptr(),
                                                 ws.numel(), L.stream_ptr(dev)), "rtkv_decode_attention_packed")
    return out


def _decode_attention_tail(p: dict, q: torch.Tensor, num_kv_heads: int, scale: Optional[float], tail: DecodeTail):
    L.require_device(p["codes_k"], p["codes_v"], q, tail.k, tail.v, tail.rows_dev)
    dev = q.device
    B, Hq, D = q.shape
    args, Sp, _keep = _packed_args("decode", p, q, B, D, num_kv_heads, dev, nullable=True)
    dt = _dense_tail(tail, q, B, num_kv_heads * D)
    out = torch.zeros(B, Hq, D, dtype=torch.float32, device=dev)
    qc = q.contiguous()
    ws = torch.empty(L.lib().rtkv_decode_tail_workspace_size(B, Hq, num_kv_heads, D, Sp, tail.capacity),
                     dtype=torch.uint8, device=dev)
    sc = float(scale) if scale is not None else 1.0 / float(D) ** 0.5
    L.check(L.lib().rtkv_decode_attention_packed_tail(*args, qc.data_ptr(), Hq, sc, ctypes.byref(dt), out.data_ptr(),
                                                      ws.data_ptr(), ws.numel(), L.stream_ptr(dev)),
            "rtkv_decode_attention_packed_tail")
    return out


def extend_attention(p: dict, q: torch.Tensor, num_kv_heads: int, tail: DecodeTail,
                     scale: Optional[float] = None) -> torch.Tensor:
    """Attention of T new tokens per batch row over a packed layer followed by the dense tail
    (rtkv_extend_attention_packed_tail).  q: [B, Hq, T, D] in the layer's dtype, post-RoPE; the tail
    already holds the T new tokens as its last T rows (append, then attend).  Returns fp32
    [B, Hq, T, D]: query t attends over every kept row and the tail rows u < max(0, n_b − (T−1−t)),
    n_b the tail's count of batch row b — causal among the new tokens, everything older fully visible,
    one softmax over the concatenation.  scale defaults to 1/sqrt(D).

    The kernel takes float16 and bfloat16 with head_dim 128.  Anything else decode_attention takes
    (float32 states, other head dims) is computed with no new kernel: T single-token steps of
    decode_attention(..., tail=) over the same buffers with device-side counts n_b − (T−1−t) clamped
    at 0 — the same result, at the cost of T decode steps."""
    L.require_device(p["codes_k"], p["codes_v"], q, tail.k, tail.v, tail.rows_dev)
    dev = q.device
    if q.dim() != 4:
        raise ValueError(f"q must be [B, Hq, T, D], got {tuple(q.shape)}")
    B, Hq, T, D = q.shape
    if T < 1:
        raise ValueError("q holds no new token (T < 1)")
    if num_kv_heads < 1 or Hq % num_kv_heads:
        raise ValueError(f"{Hq} query heads are not a multiple of {num_kv_heads} kv heads")
    if q.dtype not in (torch.float16, torch.bfloat16) or D != 128:
        # outside the kernel's envelope: T decode steps, step t seeing the tail up to its own token
        out = torch.empty(B, Hq, T, D, dtype=torch.float32, device=dev)
        n_b = tail.rows_dev.clamp(0, tail.capacity)
        for t in range(T):
            rows_t = (n_b - (T - 1 - t)).clamp_(min=0)
            out[:, :, t] = _decode_attention_tail(p, q[:, :, t], num_kv_heads, scale,
                                                  DecodeTail.from_tensors(tail.k, tail.v, rows_t))
        return out
    args, Sp, _keep = _packed_args("extend", p, q, B, D, num_kv_heads, dev, nullable=True)
    dt = _dense_tail(tail, q, B, num_kv_heads * D)
    if q.stride(3) != 1 or any(st % 8 for st in q.stride()[:3]) or q.data_ptr() % 16:
        q = q.contiguous()
    out = torch.empty(B, Hq, T, D, dtype=torch.float32, device=dev)
    ws = torch.empty(L.lib().rtkv_extend_workspace_size(B, Hq, num_kv_heads, D, T, Sp, tail.capacity), dtype=torch.uint8,
                     device=dev)
    sc = float(scale) if scale is not None else 1.0 / float(D) ** 0.5
    L.check(L.lib().rtkv_extend_attention_packed_tail(*args, q.data_ptr(), q.stride(0), q.stride(1), q.stride(2), Hq, T,
                                                      sc, ctypes.byref(dt), out.data_ptr(), ws.data_ptr(), ws.numel(),
                                                      L.stream_ptr(dev)), "rtkv_extend_attention_packed_tail")
    return out


def _gq_heads(g, q: torch.Tensor, num_kv_heads: int):
    if num_kv_heads != g.H:
        raise ValueError(f"num_kv_heads {num_kv_heads} != the gq layer's {g.H} heads of 128")
    if q.shape[0] != 1:
        raise ValueError("a gq layer holds one batch row (B = 1)")


def gq_extend_attention(g, q: torch.Tensor, num_kv_heads: int, tail: DecodeTail,
                        scale: Optional[float] = None) -> torch.Tensor:
    """extend_attention over a layer in the rtkv-gq/1 format (a GroupQuantKVCache): q [1, Hq, T, 128], the
    tail already holding the T new tokens as its last T rows; fp32 [1, Hq, T, 128], query t over every
    gq row and the tail rows u < max(0, n − (T−1−t)).  There is no multi-token gq kernel: T single-token
    steps of g.attend(..., tail=) over the same buffers with device-side counts — the fall-back
    extend_attention takes outside its kernel's envelope."""
    if q.dim() != 4:
        raise ValueError(f"q must be [1, Hq, T, 128], got {tuple(q.shape)}")
    _gq_heads(g, q, num_kv_heads)
    B, Hq, T, D = q.shape
    if T < 1:
        raise ValueError("q holds no new token (T < 1)")
    out = torch.empty(B, Hq, T, D, dtype=torch.float32, device=q.device)
    n_b = tail.rows_dev.clamp(0, tail.capacity)
    for t in range(T):
        rows_t = (n_b - (T - 1 - t)).clamp_(min=0)
        out[:, :, t] = g.attend(q[:, :, t], scale, tail=DecodeTail.from_tensors(tail.k, tail.v, rows_t))
    return out


class AdaptiveQuantization(nn.Module):
    """One scale/zero-point per precision class over all of that class's rows; bits by class index
    (compression_layers.py:96-175)."""

    def __init__(self, feature_dim: int, num_bits_options: list = [2, 4, 8]):
        super().__init__()
        self.feature_dim = feature_dim
        self.num_bits_options = num_bits_options
        self.quantization_params = {b: {"scale": torch.ones(1), "zero_point": torch.zeros(1)}
                                    for b in num_bits_options}

    def compute_quantization_params(self, tensor: torch.Tensor, num_bits: int):
        L.require_device(tensor)
        x = tensor.contiguous()
        sz = torch.empty(2, dtype=torch.float32, device=x.device)
        ws = _workspace(x.device).get(1, 1)
        L.check(L.lib().rtkv_tensor_quant_params(x.data_ptr(), L.dtype_code(x), 1, x.numel(), None, 0, int(num_bits),
                                                 sz.data_ptr(), ws.data_ptr(), ws.numel(), L.stream_ptr(x.device)),
                "rtkv_tensor_quant_params")
        return sz[0], sz[1]

    def quantize_tensor(self, tensor, num_bits, scale, zero_point):
        L.require_device(tensor)
        x = tensor.contiguous()
        sz = torch.stack([torch.as_tensor(scale, device=x.device).float().reshape(()),
                          torch.as_tensor(zero_point, device=x.device).float().reshape(())])
        out = torch.empty_like(x)
        L.check(L.lib().rtkv_tensor_fake_quant(x.data_ptr(), L.dtype_code(x), 1, x.numel(), None, 0, int(num_bits),
                                               sz.data_ptr(), out.data_ptr(), L.stream_ptr(x.device)),
                "rtkv_tensor_fake_quant")
        return out

    def forward(self, tensor: torch.Tensor, precision_labels: torch.Tensor) -> torch.Tensor:
        L.require_device(tensor, precision_labels)
        x = tensor.contiguous()
        labels = precision_labels.to(torch.uint8).contiguous()
        n_rows = labels.numel()
        row_len = x.numel() // max(n_rows, 1)
        out = torch.zeros_like(x)
        dev = x.device
        st = L.stream_ptr(dev)
        present = torch.bincount(precision_labels.reshape(-1).long().clamp(0, 255), minlength=256).tolist()
        for level, bits in enumerate(self.num_bits_options):
            if level > 255 or present[level] == 0:
                continue
            sz = torch.empty(2, dtype=torch.float32, device=dev)
            ws = _workspace(dev).get(1, 1)
            L.check(L.lib().rtkv_tensor_quant_params(x.data_ptr(), L.dtype_code(x), n_rows, row_len, labels.data_ptr(),
                                                     level, int(bits), sz.data_ptr(), ws.data_ptr(), ws.numel(), st),
                    "rtkv_tensor_quant_params")
            L.check(L.lib().rtkv_tensor_fake_quant(x.data_ptr(), L.dtype_code(x), n_rows, row_len, labels.data_ptr(),
                                                   level, int(bits), sz.data_ptr(), out.data_ptr(), st),
                    "rtkv_tensor_fake_quant")
        return out
