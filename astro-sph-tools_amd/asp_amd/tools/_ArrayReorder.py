"""Cross-snapshot ID matching on the GPU, mirroring the reference module
tools/_ArrayReorder.py: ``ArrayReorder`` (:815-1038) and ``ArrayMapping`` (:1042-1171).

The reference lines two ID orderings up with argsort / isin / searchsorted on the host
(:1003-1038, :1057-1081) and copies every field with a fancy index (:957, :1129).  Here the
match is one call of ``asp_match_ids`` (a partitioned hash join, csrc/asp_match.hip) and
every field one call of ``asp_take_rows``.  For source IDs S (filter sf) and target IDs T
(filter tf):

    index[j]          = the i with sf[i], tf[j] and S[i] == T[j], or -1
    source_matched[i] = sf[i] and some j with tf[j] has T[j] == S[i]

so that ``ArrayReorder.create(S, T, sf, tf)(data, default_value=d)`` is
``where(index >= 0, data[index], d)``, ``.source_filter`` / ``.target_filter`` are
``source_matched`` / ``index >= 0`` and ``.reverse`` is the same with the roles swapped
(tests/reorder_ref.py restates this in NumPy; tests/golden/g12_array_reorder.npz pins it to
the reference's own objects).  NumPy inputs give NumPy results; torch tensors on the GPU
stay there, on the current or the given stream.  There is no CPU fallback.

``ArrayReorder_2`` and the MPI variants (:88-813) are not mirrored: one process per GPU.
Unit-carrying arrays are handled as in ``_periodic_box_manipulations`` (duck-typed on
``.value`` / ``.units`` / ``.to``): values in the source data's unit, rewrapped.
"""
from __future__ import annotations

import numpy as np

from .. import _lib
from .._call import alloc_out, call_flags, is_device, stream_scope
from ._periodic_box_manipulations import _has_units, _in, _wrap

_MODES = {"mapping": _lib.ASP_MATCH_MAPPING, "reorder": _lib.ASP_MATCH_REORDER}

_NO_DEFAULT = ("More output elements expected than matches but no default value provided and "
               "no output target array to write matches to.")
_DUPLICATES = ("Duplicate matched detected in filtered source array. Source ID array must contain "
               "unique elements (after optional filter is applied).")


def _host_ids(x, name):
    a = np.asarray(x.cpu().numpy() if hasattr(x, "is_cuda") else x)
    if a.ndim != 1:
        raise ValueError(f"{name} must be one-dimensional, got shape {a.shape}")
    if a.dtype.kind not in "iu":
        raise ValueError(f"{name} must be integer IDs, got {a.dtype}")
    if a.dtype == np.uint64:
        return np.ascontiguousarray(a).view(np.int64)  # the same 64 bits
    return np.ascontiguousarray(a, dtype=np.int64)


def _device_ids(x, name, dev):
    import torch
    if not hasattr(x, "is_cuda"):
        return torch.from_numpy(_host_ids(x, name)).to(dev)
    if x.dim() != 1:
        raise ValueError(f"{name} must be one-dimensional, got shape {tuple(x.shape)}")
    if x.dtype.is_floating_point or x.dtype.is_complex or x.dtype == torch.bool:
        raise ValueError(f"{name} must be integer IDs, got {x.dtype}")
    x = x.to(dev)
    if x.dtype == torch.int64:
        return x.contiguous()
    if x.dtype == getattr(torch, "uint64", None):
        return x.contiguous().view(torch.int64)
    return x.to(torch.int64).contiguous()


def _host_filter(f, n, name):
    if f is None:
        return None
    a = np.asarray(f.cpu().numpy() if hasattr(f, "is_cuda") else f)
    if a.dtype != np.bool_ or a.shape != (n,):
        raise ValueError(f"{name} must be a boolean array of length {n}, got {a.dtype} {a.shape}")
    return np.ascontiguousarray(a).view(np.uint8)


def _device_filter(f, n, name, dev):
    import torch
    if f is None:
        return None
    if not hasattr(f, "is_cuda"):
        return torch.from_numpy(_host_filter(f, n, name)).to(dev)
    if f.dtype != torch.bool or tuple(f.shape) != (n,):
        raise ValueError(f"{name} must be a boolean tensor of length {n}, got {f.dtype} "
                         f"{tuple(f.shape)}")
    return f.to(dev).contiguous().view(torch.uint8)


def match_ids(source_ids, target_ids, source_filter=None, target_filter=None, *,
              mode="mapping", device: int = 0, stream=None):
    """``(index, source_matched, counts)`` of the module docstring.

    ``index``: int32, one per target; ``source_matched``: bool, one per source; ``counts``:
    ``(targets matched, sources matched, duplicates seen)`` as Python ints.  A duplicate is
    an ID carried by two or more filtered sources and asked for by a filtered target; with
    ``counts[2] != 0`` the two arrays are unspecified (the classes below raise).  IDs: int64
    or uint64 (reinterpreted), other integer types converted; floats are refused.  NumPy
    arrays in, NumPy arrays out; integer torch tensors on the GPU in, tensors there out,
    ordered on the current or the given stream (the call waits for the counts).
    """
    if mode not in _MODES:
        raise ValueError(f"mode must be 'mapping' or 'reorder', got {mode!r}")
    counts = (_lib.C.c_int64 * 3)()
    if is_device(source_ids) or is_device(target_ids):
        import torch
        dev = source_ids.device if is_device(source_ids) else target_ids.device
        with stream_scope(dev, stream) as scope:  # conversions and uploads ordered on the stream
            S = _device_ids(source_ids, "source_ids", dev)
            T = _device_ids(target_ids, "target_ids", dev)
            ns, nt = S.numel(), T.numel()
            sf = _device_filter(source_filter, ns, "source_filter", dev)
            tf = _device_filter(target_filter, nt, "target_filter", dev)
            index = alloc_out((nt,), torch.int32, dev)
            matched = alloc_out((ns,), torch.uint8, dev, zeros=True)
            scope.keep(S, T, sf, tf, index, matched)
            _lib.check(_lib.lib().asp_match_ids(
                _lib.ptr(S, _lib._i64), _lib.ptr(sf, _lib._u8), ns, _lib.ptr(T, _lib._i64),
                _lib.ptr(tf, _lib._u8), nt, _MODES[mode], _lib.ptr(index, _lib._i32),
                _lib.ptr(matched, _lib._u8), counts, call_flags(device_ptrs=True),
                dev.index or 0, scope.raw))
            matched = matched.view(torch.bool)
        return index, matched, tuple(int(c) for c in counts)
    S = _host_ids(source_ids, "source_ids")
    T = _host_ids(target_ids, "target_ids")
    ns, nt = S.shape[0], T.shape[0]
    sf = _host_filter(source_filter, ns, "source_filter")
    tf = _host_filter(target_filter, nt, "target_filter")
    if ns > 0 and nt > 0:
        _lib.require_gpu(device)
    index = np.empty(nt, dtype=np.int32)
    matched = np.zeros(ns, dtype=np.uint8)
    _lib.check(_lib.lib().asp_match_ids(
        _lib.ptr(S, _lib._i64), _lib.ptr(sf, _lib._u8), ns, _lib.ptr(T, _lib._i64),
        _lib.ptr(tf, _lib._u8), nt, _MODES[mode], _lib.ptr(index, _lib._i32),
        _lib.ptr(matched, _lib._u8), counts, 0, device, None))
    return index, matched.view(np.bool_), tuple(int(c) for c in counts)


def _void(a):
    return None if a is None else _lib.C.c_void_p(a.data_ptr() if hasattr(a, "data_ptr")
                                                  else a.ctypes.data)


def take_rows(data, index, output_array=None, default_value=None, *, device: int = 0,
              stream=None):
    """``out[j] = data[index[j]]`` for ``index[j] >= 0``; other rows get ``default_value``
    (broadcast to one row), or keep ``output_array``'s contents when there is no default
    (uninitialised for a fresh output).  Rows are ``data[i]``: trailing dimensions move as one
    row of bytes.  Host arrays or device tensors (``data`` decides); an ``index >= len(data)``
    raises ValueError.  Returns the output."""
    if is_device(data):
        import torch
        dev = data.device
        with stream_scope(dev, stream) as scope:
            src = data.contiguous()
            idx = index if hasattr(index, "is_cuda") else torch.from_numpy(
                np.ascontiguousarray(index, dtype=np.int32))
            idx = idx.to(dev)
            if idx.dtype != torch.int32:
                idx = idx.to(torch.int32)
            idx = idx.contiguous()
            n_index, row_shape = idx.numel(), tuple(src.shape[1:])
            out = output_array
            if out is None:
                out = torch.empty((n_index,) + row_shape, dtype=src.dtype, device=dev)
            elif (not is_device(out) or out.dtype != src.dtype or not out.is_contiguous()
                  or tuple(out.shape) != (n_index,) + row_shape):
                raise ValueError("output_array must be a contiguous device tensor of the data's "
                                 f"dtype and shape {(n_index,) + row_shape}")
            fill = None
            if default_value is not None:
                fill = torch.as_tensor(default_value, dtype=src.dtype, device=dev)
                fill = fill.broadcast_to(row_shape).contiguous()
            scope.keep(src, idx, fill, out)
            row_bytes = src.element_size() * int(np.prod(row_shape, dtype=np.int64))
            _lib.check(_lib.lib().asp_take_rows(
                _void(src), src.shape[0], row_bytes, _lib.ptr(idx, _lib._i32), n_index,
                _void(fill), _void(out), call_flags(device_ptrs=True), dev.index or 0, scope.raw))
        return out
    src = np.ascontiguousarray(data)
    if src.ndim < 1:
        raise ValueError("data must have at least one dimension")
    idx = np.ascontiguousarray(index.cpu().numpy() if hasattr(index, "is_cuda") else index,
                               dtype=np.int32)
    n_index, row_shape = idx.shape[0], src.shape[1:]
    out = output_array
    if out is None:
        out = np.empty((n_index,) + row_shape, dtype=src.dtype)
    elif (not isinstance(out, np.ndarray) or out.dtype != src.dtype or not out.flags.c_contiguous
          or out.shape != (n_index,) + row_shape):
        raise ValueError("output_array must be a C-contiguous array of the data's dtype and "
                         f"shape {(n_index,) + row_shape}")
    fill = None
    if default_value is not None:
        fill = np.ascontiguousarray(np.broadcast_to(np.asarray(default_value, dtype=src.dtype),
                                                    row_shape))
    row_bytes = src.dtype.itemsize * int(np.prod(row_shape, dtype=np.int64))
    if n_index > 0:
        _lib.require_gpu(device)
    _lib.check(_lib.lib().asp_take_rows(_void(src), src.shape[0], row_bytes,
                                        _lib.ptr(idx, _lib._i32), n_index, _void(fill),
                                        _void(out), 0, device, None))
    return out


class _Matched:
    """What both classes share: the match, its filters and the call."""

    _mode = "mapping"

    def __init__(self, index, source_matched, counts, _inputs=None):
        self._index = index
        self._source_matched = source_matched
        self._counts = tuple(int(c) for c in counts)
        self._inputs = _inputs  # (source, target, source filter, target filter, device, stream)
        self._input_length = int(source_matched.shape[0])
        self._output_length = int(index.shape[0])
        self._n_matched = self._counts[0]
        self._target_matched = None
        self._result_is_exact = self._output_length == self._n_matched

    @property
    def input_length(self) -> int:
        return self._input_length

    @property
    def output_length(self) -> int:
        return self._output_length

    def _target_filter(self):
        if self._target_matched is None:
            self._target_matched = self._index >= 0
        return self._target_matched

    def __call__(self, source_data, output_array=None, default_value=None):
        """Reorder data (reference :933-959, :1107-1131)."""
        if not self._result_is_exact and output_array is None and default_value is None:
            raise ValueError(_NO_DEFAULT)
        if _has_units(source_data):  # the reference's unyt overload (:961-985, :1133-1157)
            units = source_data.units
            raw_default = None if default_value is None else _in(default_value, units)
            values = source_data.value
            if output_array is None:
                return _wrap(source_data, self(values, None, raw_default), units)
            raw = np.full(output_array.shape, np.nan, dtype=np.asarray(values).dtype)
            self(values, raw, raw_default)
            mask = np.asarray(self._target_filter().cpu() if hasattr(self._index, "is_cuda")
                              else self._target_filter())
            output_array[mask] = _wrap(source_data, raw[mask], units).to(output_array.units)
            if default_value is not None:
                output_array[~mask] = _wrap(source_data, raw[~mask], units).to(output_array.units)
            return output_array
        kw = {}
        if self._inputs is not None:
            kw = dict(device=self._inputs[4], stream=self._inputs[5])
        return take_rows(source_data, self._index, output_array, default_value, **kw)

    @classmethod
    def _create(cls, source, target, source_filter, target_filter, device, stream):
        index, matched, counts = match_ids(source, target, source_filter, target_filter,
                                           mode=cls._mode, device=device, stream=stream)
        return cls(index, matched, counts,
                   _inputs=(source, target, source_filter, target_filter, device, stream))


class ArrayReorder(_Matched):
    """Callable that rearranges the elements of an array into the order of a template array
    (reference :815-1038).  Build it with ``create``; ``reverse`` is the opposite operation."""

    _mode = "reorder"

    def __init__(self, index, source_matched, counts, _inputs=None):
        super().__init__(index, source_matched, counts, _inputs)
        n_target, n_source, n_dup = self._counts
        if n_dup != 0 or n_target != n_source:  # (:836-838, with the message it intends)
            raise ValueError("Source and destination filters select a different number of items "
                             f"({n_source} and {n_target}).")
        self._reverse = None

    @staticmethod
    def create(source_order, target_order, source_order_filter=None, target_order_filter=None, *,
               device: int = 0, stream=None) -> "ArrayReorder":
        """A new ArrayReorder; the filters let only some elements take part in the matching
        without altering the input or output shapes (:988-1038)."""
        return ArrayReorder._create(source_order, target_order, source_order_filter,
                                    target_order_filter, device, stream)

    @property
    def reverse(self) -> "ArrayReorder":
        """The reverse operation: one further match with the roles swapped, made on first use."""
        if self._reverse is None:
            if self._inputs is None:
                raise ValueError("this ArrayReorder was not built by create(): no IDs to reverse")
            s, t, sf, tf, device, stream = self._inputs
            self._reverse = ArrayReorder._create(t, s, tf, sf, device, stream)
            self._reverse._reverse = self
        return self._reverse

    @property
    def source_filter(self):
        return self._source_matched

    @property
    def target_filter(self):
        return self._target_filter()

    def __len__(self) -> int:
        return self.input_length

    @property
    def matched_items(self) -> int:
        return self._n_matched

    @property
    def uses_all_inputs(self) -> bool:
        """All inputs are matches."""
        return self._input_length == self._n_matched

    @property
    def all_outputs_matched(self) -> bool:
        """All outputs are matches."""
        return self._result_is_exact

    @property
    def lossless(self) -> bool:
        """All outputs are inputs and all inputs are outputs."""
        return self.uses_all_inputs and self._result_is_exact

    @property
    def matches_are_reduction(self) -> bool:
        """Fewer matches than the number of inputs."""
        return self._input_length > self._n_matched

    @property
    def results_are_expansion(self) -> bool:
        """More outputs than the number of matches."""
        return self._output_length > self._n_matched

    @property
    def results_are_subset(self) -> bool:
        """Outputs are a subset of the inputs."""
        return self.matches_are_reduction and self._result_is_exact

    @property
    def results_are_superset(self) -> bool:
        """Outputs are a superset of the inputs."""
        return self.results_are_expansion and self.uses_all_inputs


class ArrayMapping(_Matched):
    """Callable one-way mapping of data from a source order onto a target order: the source
    IDs are unique, the target may repeat them (reference :1042-1171)."""

    _mode = "mapping"

    def __init__(self, index, source_matched, counts, _inputs=None):
        super().__init__(index, source_matched, counts, _inputs)
        if self._counts[2] != 0:  # (:1074-1075)
            raise IndexError(_DUPLICATES)

    @staticmethod
    def create(source_IDs, target_IDs, source_ID_filter=None, target_ID_filter=None, *,
               device: int = 0, stream=None) -> "ArrayMapping":
        return ArrayMapping._create(source_IDs, target_IDs, source_ID_filter, target_ID_filter,
                                    device, stream)

    @property
    def input_filter(self):
        return self._source_matched

    @property
    def output_filter(self):
        return self._target_filter()
