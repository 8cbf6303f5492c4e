"""stringzilla_amd - the MI355X-native build of StringZillas' batched similarity engines, Python side.

Mirrors the reference's `stringzillas` Python module for this hot path - same class names, constructor arguments,
call convention and result dtypes (/root/reference/python/README.md:452-560, python/stringzillas/similarities.c) -
on top of the C-ABI of `libstringzillas_rocm_shared.so`:

    import stringzilla_amd as szs
    gpu = szs.DeviceScope(gpu_device=0)
    engine = szs.LevenshteinDistances(capabilities=gpu)
    distances = engine(szs.Strs(["hello", "world"]), szs.Strs(["hallo", "word"]), device=gpu)   # 2x2 uint64

Every score is computed by hand-written gfx950 kernels behind the C-ABI.  There is no CPU path: without the shared
library, or without a GPU, construction fails loudly.  PyTorch is used only to own device memory.
"""

from __future__ import annotations

import ctypes
from typing import Iterable, Optional, Sequence, Union

import numpy as np

from . import _abi
from ._abi import CallProfile, StringZillasError, lib

__all__ = [
    "DeviceScope", "Strs", "LevenshteinDistances", "LevenshteinDistancesUTF8", "NeedlemanWunschScores",
    "SmithWatermanScores", "Fingerprints", "StringZillasError", "to_device", "Node", "NodeEngine", "__capabilities__",
    "__version__",
]

__version__ = f"{lib.szs_version_major()}.{lib.szs_version_minor()}.{lib.szs_version_patch()}"


def _capability_names(mask: int) -> tuple:
    names = []
    if mask & _abi.CAP_SERIAL:
        names.append("serial")
    if mask & _abi.CAP_CUDA:
        names.append("cuda")  # the reference's name for "a GPU engine exists"; on this build it means HIP/gfx950
    return tuple(names)


__capabilities__ = _capability_names(lib.szs_capabilities())


def _capability_mask(capabilities) -> int:
    """Accepts what the reference accepts: None, a tuple of names, or a DeviceScope (README.md:492)."""
    if capabilities is None:
        return lib.szs_capabilities()
    if isinstance(capabilities, DeviceScope):
        return capabilities.capabilities_mask
    mask = 0
    for name in capabilities:
        if name == "serial":
            mask |= _abi.CAP_SERIAL
        elif name == "parallel":
            mask |= _abi.CAP_PARALLEL
        elif name in ("cuda", "rocm", "hip"):
            mask |= _abi.CAP_CUDA
        else:
            raise ValueError(f"Unknown capability {name!r}")
    return mask


class DeviceScope:
    """`DeviceScope(cpu_cores=None, gpu_device=None)` - where engine calls run (README.md:458-470)."""

    def __init__(self, cpu_cores: Optional[int] = None, gpu_device: Optional[int] = None):
        if cpu_cores is not None and gpu_device is not None:
            raise ValueError("Cannot specify both cpu_cores and gpu_device")
        handle, error = ctypes.c_void_p(), ctypes.c_char_p()
        if gpu_device is not None:
            status = lib.szs_device_scope_init_gpu_device(gpu_device, ctypes.byref(handle), ctypes.byref(error))
        elif cpu_cores is not None:
            status = lib.szs_device_scope_init_cpu_cores(cpu_cores, ctypes.byref(handle), ctypes.byref(error))
        else:
            status = lib.szs_device_scope_init_default(ctypes.byref(handle), ctypes.byref(error))
        _abi.check(status, error)
        self.handle = handle
        self.gpu_device = gpu_device
        self.cpu_cores = cpu_cores

    @property
    def capabilities_mask(self) -> int:
        mask, error = ctypes.c_int(), ctypes.c_char_p()
        _abi.check(lib.szs_device_scope_get_capabilities(self.handle, ctypes.byref(mask), ctypes.byref(error)), error)
        return mask.value

    @property
    def capabilities(self) -> tuple:
        return _capability_names(self.capabilities_mask)

    def __del__(self):
        handle = getattr(self, "handle", None)
        if handle and lib is not None:  # `lib` is gone when the interpreter is tearing the module down
            lib.szs_device_scope_free(handle)
            self.handle = None


_default_scope: Optional[DeviceScope] = None


def _get_default_scope() -> DeviceScope:
    global _default_scope
    if _default_scope is None:
        _default_scope = DeviceScope()
    return _default_scope


class Strs:
    """An Arrow-like tape of byte strings - the stand-in for the reference's `stringzilla.Strs` (a tape is what the
    binding hands to `szs_*_u32tape` / `_u64tape`: python/stringzillas/similarities.c:275-318).

    The tape is assembled on the host and moved to device memory on first use (the reference's binding swaps the
    collection to its unified allocator at the same point: similarities.c:268-272).  A tape that was BORN on a device
    (`from_device`: the receiving side of an RCCL broadcast) keeps its bytes there; only the offsets - which the host
    planner and the row dealer read - are mirrored on the host, the bytes are downloaded if somebody asks for them."""

    def __init__(self, strings: Iterable[Union[str, bytes, bytearray, memoryview]] = (), wide_offsets: bool = False):
        encoded = [s.encode("utf-8") if isinstance(s, str) else bytes(s) for s in strings]
        total = sum(len(s) for s in encoded)
        self.wide_offsets = bool(wide_offsets or total >= 2**32)
        self.count = len(encoded)
        offsets = np.zeros(self.count + 1, dtype=np.uint64 if self.wide_offsets else np.uint32)
        if self.count:
            np.cumsum(np.fromiter((len(s) for s in encoded), dtype=np.uint64, count=self.count), out=offsets[1:])
        self.offsets = offsets
        self._data = np.frombuffer(b"".join(encoded), dtype=np.uint8).copy() if total else np.zeros(1, np.uint8)
        self._device = None  # (device index or "cpu", data tensor, offsets tensor)

    @classmethod
    def from_tape(cls, data: np.ndarray, offsets: np.ndarray) -> "Strs":
        self = cls.__new__(cls)
        self._data = np.ascontiguousarray(data, dtype=np.uint8) if data.size else np.zeros(1, np.uint8)
        self.offsets = np.ascontiguousarray(offsets)
        assert self.offsets.dtype in (np.uint32, np.uint64)
        self.wide_offsets = self.offsets.dtype == np.uint64
        self.count = len(offsets) - 1
        self._device = None
        return self

    @classmethod
    def from_device(cls, data, offsets) -> "Strs":
        """A tape whose bytes (`uint8` tensor) and offsets (`int32` / `int64` tensor holding the unsigned values) already
        live in torch memory - device memory after an RCCL broadcast, host memory under `gloo`."""
        self = cls.__new__(cls)
        self._data = None
        self.wide_offsets = offsets.element_size() == 8
        self.offsets = offsets.cpu().numpy().view(np.uint64 if self.wide_offsets else np.uint32)
        self.count = len(self.offsets) - 1
        self._device = (data.device.index if data.device.type == "cuda" else "cpu", data, offsets)
        return self

    @property
    def data(self) -> np.ndarray:
        if self._data is None:  # born on a device: download on demand
            host = self._device[1].cpu().numpy()
            self._data = host if host.size else np.zeros(1, np.uint8)
        return self._data

    def __len__(self) -> int:
        return self.count

    def __getitem__(self, index: int) -> bytes:
        return self.data[int(self.offsets[index]):int(self.offsets[index + 1])].tobytes()

    def lengths(self) -> np.ndarray:
        return np.diff(self.offsets.astype(np.int64))

    def select(self, rows: np.ndarray) -> "Strs":
        """Sub-tape holding `rows` of this tape, in that order; gathered where the bytes live (on the device for a
        device-born tape: one index computation and one gather, nothing crosses the host link)."""
        rows = np.asarray(rows, dtype=np.int64)
        offsets = self.offsets.astype(np.int64)
        starts, lengths = offsets[rows], offsets[rows + 1] - offsets[rows]
        new_offsets = np.zeros(len(rows) + 1, dtype=self.offsets.dtype)
        np.cumsum(lengths, out=new_offsets[1:])
        total = int(new_offsets[-1])
        if self._data is None and self._device is not None:
            import torch

            _, data, _ = self._device
            if total:
                shift = torch.from_numpy(np.repeat(starts - new_offsets[:-1].astype(np.int64), lengths)).to(data.device)
                gathered = data[torch.arange(total, device=data.device) + shift]
            else:
                gathered = torch.zeros(1, dtype=torch.uint8, device=data.device)
            signed = torch.from_numpy(new_offsets.view(np.int64 if self.wide_offsets else np.int32)).to(data.device)
            return Strs.from_device(gathered, signed)
        if total:
            index = np.arange(total, dtype=np.int64) + np.repeat(starts - new_offsets[:-1].astype(np.int64), lengths)
            return Strs.from_tape(self.data[index], new_offsets)
        return Strs.from_tape(np.zeros(1, np.uint8), new_offsets)

    def to_device(self, gpu_device: int = 0) -> "Strs":
        if self._device is None or self._device[0] != gpu_device:
            import torch

            if not torch.cuda.is_available():
                raise RuntimeError("stringzilla_amd needs a GPU: torch.cuda.is_available() is False (no CPU fallback)")
            where = torch.device("cuda", gpu_device)
            if self._device is not None and self._data is None:  # born elsewhere: move the tensors
                self._device = (gpu_device, self._device[1].to(where), self._device[2].to(where))
                return self
            data = torch.from_numpy(self.data).to(where)
            # torch has no uint32/uint64 arithmetic, but plain storage is all we need: view as signed of equal width.
            signed = self.offsets.view(np.int64 if self.wide_offsets else np.int32)
            offsets = torch.from_numpy(signed).to(where)
            self._device = (gpu_device, data, offsets)
        return self

    def _tape(self, gpu_device: int):
        self.to_device(gpu_device)
        _, data, offsets = self._device
        tape_type = _abi.U64Tape if self.wide_offsets else _abi.U32Tape
        return tape_type(data.data_ptr(), offsets.data_ptr(), self.count)


def to_device(strs: Strs, gpu_device: int = 0) -> Strs:
    """Module-level `szs.to_device(strs)` of the reference (README.md:560): forces device residency now."""
    return strs.to_device(gpu_device)


def _as_strs(collection) -> Strs:
    return collection if isinstance(collection, Strs) else Strs(collection)


def _array_facts(array, name):
    """-> (shape, item size, byte strides, pointer, GPU index or None) of a NumPy array or a torch tensor; ValueError for anything else.
    The one place that asks "NumPy or torch?": what an argument must look like stays its caller's rule."""
    if isinstance(array, np.ndarray):
        return array.shape, array.dtype.itemsize, array.strides, array.ctypes.data, None
    if type(array).__module__.partition(".")[0] == "torch" and hasattr(array, "data_ptr"):
        itemsize = array.element_size()
        return (tuple(array.shape), itemsize, tuple(stride * itemsize for stride in array.stride()), array.data_ptr(),
                array.device.index if array.is_cuda else None)
    raise ValueError(f"`{name}` must be a NumPy array or a torch tensor, got {type(array).__name__}")


def _listed_cells(matrix, name, shape_wanted):
    """A `(rows, k)` matrix of 8-byte cells with contiguous rows, as `rerank` and `fuzzy_find` take them -> (pointer, row stride in
    cells, shape); ValueError otherwise."""
    shape, itemsize, strides, pointer, _ = _array_facts(matrix, name)
    if len(shape) != 2 or shape[1] < 1 or (shape_wanted is not None and shape != shape_wanted) or itemsize != 8 or any(
            stride % 8 for stride in strides) or (shape[1] > 1 and strides[1] != 8) or (shape[0] > 1 and strides[0] < shape[1] * 8):
        raise ValueError(f"`{name}` must be a (rows, k) matrix of 8-byte cells with contiguous rows, k at least 1")
    return pointer, strides[0] // 8 if shape[0] > 1 else shape[1], shape


def _cells_of_one_stride(named, shape, stride=None):
    """`_listed_cells` of every (name, matrix) of `named`, which must share one row stride - `stride`, where one is given ->
    (pointers, that stride)."""
    pointers = []
    for name, matrix in named:
        pointer, own_stride, _ = _listed_cells(matrix, name, shape)
        if stride is not None and own_stride != stride:
            raise ValueError(f"`{name}` must share the row stride of the other matrices of the call")
        stride = own_stride
        pointers.append(pointer)
    return pointers, stride


def _vector_cells(array, name, rows):
    """A contiguous vector of `rows` 8-byte cells -> its pointer; ValueError otherwise."""
    shape, itemsize, strides, pointer, _ = _array_facts(array, name)
    if shape != (rows,) or itemsize != 8 or (rows > 1 and strides != (8,)):
        raise ValueError(f"`{name}` must be a contiguous vector of {rows} 8-byte cells")
    return pointer


def _named_out(out, names):
    """`out` as ((name, array), ...): a tuple or a list with one array per name of `names`; ValueError otherwise."""
    if not isinstance(out, (tuple, list)) or len(out) != len(names):
        raise ValueError(f"`out` must be a tuple ({', '.join(names)})")
    return tuple(zip(("out " + name for name in names), out))


def _top_k_out(out, second, shape):
    """The `out=(indices, second)` of a `top_k`, `second` may be None -> (indices pointer, second pointer or None, row stride,
    ((name, array), ...)); ValueError otherwise."""
    try:
        named = (("out indices", out[0]), ("out " + second, out[1]))
    except (TypeError, IndexError, KeyError):
        raise ValueError(f"`out` must be a pair (indices, {second})") from None
    if named[0][1] is None:
        raise ValueError("`out indices` must not be None")
    pointers, stride = _cells_of_one_stride(named if named[1][1] is not None else named[:1], shape)
    return pointers[0], pointers[1] if len(pointers) > 1 else None, stride, named


def _integer(value, name, low, high=None):
    """`value` as an `int` within [low, high] (`high` None: no upper end); ValueError for a bool, for anything that is no integer, and
    outside the range."""
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)) or int(value) < low or (
            high is not None and int(value) > high):
        raise ValueError(f"{name} must be an integer within [{low}, {'...' if high is None else high}], got {value!r}")
    return int(value)


def _text_bytes(text):
    """The `text` of a scan, checked without a GPU: bytes-like -> a NumPy view of its bytes; a contiguous `uint8` vector, NumPy or
    torch -> itself; ValueError otherwise."""
    if isinstance(text, (bytes, bytearray, memoryview)):
        return np.frombuffer(text, dtype=np.uint8)
    try:
        shape, _, strides, _, _ = _array_facts(text, "text")
    except ValueError:
        raise ValueError(f"`text` must be bytes-like, a NumPy uint8 array or a torch uint8 tensor, got {type(text).__name__}") from None
    if str(text.dtype) not in ("uint8", "torch.uint8") or len(shape) != 1 or (shape[0] > 1 and strides[0] != 1):
        raise ValueError("`text` must be a contiguous vector of uint8")
    return text


def _text_on_gpu(text, gpu_device):
    """What `_text_bytes` returned as a tensor on the call's GPU: a tensor already there goes as it is, host data is uploaded once."""
    import torch

    if isinstance(text, np.ndarray):
        text = torch.from_numpy(text if text.flags.writeable else np.array(text, copy=True))
    if not text.is_cuda:
        where = torch.device("cuda", gpu_device)
        text = text.to(where)
        torch.cuda.current_stream(where).synchronize()
    return text


def _where(engine, device):
    """-> (scope, GPU index) of a call.  The three `__call__` bodies keep their own copy of this and of what follows: they are timed."""
    scope = device or engine._scope or _get_default_scope()
    return scope, scope.gpu_device if scope.gpu_device is not None else 0


def _same_flavour(queries, candidates):
    """Both sides must use one tape flavour per call, like the binding's detection order (similarities.c:275-318) -> the pair with
    one offset width."""
    if candidates is not None and queries.wide_offsets != candidates.wide_offsets:
        queries, candidates = (Strs.from_tape(side.data, side.offsets.astype(np.uint64)) for side in (queries, candidates))
    return queries, candidates


def _on_call_gpu(named_arrays, gpu_device):
    """A device tensor goes to the kernel as a raw pointer: one on another GPU than the call's is refused (ValueError).  Whatever torch
    still has in flight for one on this GPU (a fill, say) runs on TORCH's stream, the call on the scope's own: the former is drained,
    once, or a late fill overwrites what the call wrote.  `named_arrays`: (name, array or None) pairs, host arrays among them."""
    drain = False
    for name, array in named_arrays:
        if getattr(array, "is_cuda", False):
            if array.device.index != gpu_device:
                raise ValueError(f"`{name}` is on {array.device}, the call runs on GPU {gpu_device}")
            drain = True
    if drain:
        import torch

        torch.cuda.current_stream(gpu_device).synchronize()


_ONE_SIDED = object()  # the `candidates` of `_tape_call` for an entry that takes one tape


def _tape_call(entry, scope, handle, queries, candidates, gpu_device, *arguments):
    """Calls `entry`'s `_u32tape` or `_u64tape` form - by the offsets of `queries`, which `candidates` (None: NULL) share - with
    `arguments` behind the tapes, and raises what it reports."""
    call = getattr(lib, entry + ("_u64tape" if queries.wide_offsets else "_u32tape"))
    tapes = [ctypes.byref(queries._tape(gpu_device))]
    if candidates is not _ONE_SIDED:
        tapes.append(None if candidates is None else ctypes.byref(candidates._tape(gpu_device)))
    error = ctypes.c_char_p()
    _abi.check(call(handle, scope.handle, *tapes, *arguments, ctypes.byref(error)), error)


class _Engine:
    """Shared call path: `engine(queries, candidates=None, device=None, out=None)` (README.md:472-482)."""

    _free = None
    _call_u32 = None
    _call_u64 = None
    _dtype = np.uint64

    def __init__(self):
        self.handle = ctypes.c_void_p()
        self._scope: Optional[DeviceScope] = None
        self._mask = 0

    def _remember(self, capabilities):
        self._mask = _capability_mask(capabilities)
        if isinstance(capabilities, DeviceScope):
            self._scope = capabilities

    @property
    def __capabilities__(self) -> tuple:
        return _capability_names(self._mask & lib.szs_capabilities())

    def last_call_profile(self) -> CallProfile:
        profile = CallProfile()
        if lib.szs_rocm_last_call_profile(self.handle, ctypes.byref(profile)) != 0:
            raise RuntimeError("engine is not initialized")
        return profile

    def __call__(self, queries, candidates=None, device: Optional[DeviceScope] = None, out=None):
        import torch

        scope = device or self._scope or _get_default_scope()
        gpu_device = scope.gpu_device if scope.gpu_device is not None else 0
        queries = _as_strs(queries)
        candidates = None if candidates is None else _as_strs(candidates)
        if queries.wide_offsets != (candidates.wide_offsets if candidates is not None else queries.wide_offsets):
            # both sides must use one tape flavour per call, like the binding's detection order (similarities.c:275-318)
            queries = Strs.from_tape(queries.data, queries.offsets.astype(np.uint64))
            candidates = Strs.from_tape(candidates.data, candidates.offsets.astype(np.uint64))
        rows = len(queries)
        columns = rows if candidates is None else len(candidates)

        error = ctypes.c_char_p()
        call = self._call_u64 if queries.wide_offsets else self._call_u32
        torch_dtype = torch.int64  # 8-byte cells; uint64 results are reinterpreted on the way out
        if out is None:
            results = torch.empty((rows, max(columns, 1)), dtype=torch_dtype, device=torch.device("cuda", gpu_device))
            results = results[:, :columns]
            pointer, stride = results.data_ptr(), max(columns, 1)
        elif isinstance(out, np.ndarray):
            if out.shape != (rows, columns) or out.dtype.itemsize != 8 or out.strides[1] != 8:
                raise ValueError("`out` must be a (rows, columns) matrix of 8-byte cells with contiguous rows")
            results, pointer, stride = out, out.ctypes.data, out.strides[0] // 8
        else:  # a torch tensor, host or device
            if tuple(out.shape) != (rows, columns) or out.element_size() != 8 or (columns and out.stride(1) != 1):
                raise ValueError("`out` must be a (rows, columns) matrix of 8-byte cells with contiguous rows")
            if out.is_cuda:  # whatever torch still has in flight for this matrix (a fill, say) runs on TORCH's stream; the scoring
                # launches run on the scope's own: drain the former, or a late fill overwrites cells the call has already scored
                torch.cuda.current_stream(out.device).synchronize()
            results, pointer, stride = out, out.data_ptr(), out.stride(0) if rows > 1 else max(columns, 1)

        q_tape = queries._tape(gpu_device)
        c_tape = None if candidates is None else candidates._tape(gpu_device)
        status = call(self.handle, scope.handle, ctypes.byref(q_tape), None if c_tape is None else ctypes.byref(c_tape),
                      pointer, stride, ctypes.byref(error))
        _abi.check(status, error)
        if out is not None:
            return out
        return results.cpu().numpy().view(self._dtype)

    def top_k(self, queries, candidates=None, k=None, device: Optional[DeviceScope] = None, out=None):
        """The `k` best candidates of every query (`szs_rocm_top_k_*`) without the full matrix: returns `(indices, scores)`, a
        `uint64` and an engine-dtype `(rows, k)` NumPy matrix, or fills `out=(indices, scores)` (NumPy arrays or torch tensors of
        8-byte cells, one row stride; `scores` may be None).  Distances rank ascending, NW / SW scores descending, ties go to the
        lower candidate index.  `candidates` None: self-search, each query's own index excluded.  A row with fewer than `k`
        candidates ends in index 2**64 - 1 and score 0."""
        import torch

        k = _integer(k, "k", 1, 1024)
        queries = _as_strs(queries)
        candidates = None if candidates is None else _as_strs(candidates)
        rows, named = len(queries), ()
        if out is not None:
            indices_pointer, scores_pointer, stride, named = _top_k_out(out, "scores", (rows, k))
        scope, gpu_device = _where(self, device)
        _on_call_gpu(named, gpu_device)
        queries, candidates = _same_flavour(queries, candidates)
        if out is None:
            both = torch.empty((2, max(rows, 1), k), dtype=torch.int64, device=torch.device("cuda", gpu_device))
            indices_pointer, scores_pointer, stride = both[0].data_ptr(), both[1].data_ptr(), k
        _tape_call("szs_rocm_top_k", scope, self.handle, queries, candidates, gpu_device, k, indices_pointer, scores_pointer, stride)
        if out is not None:
            return out
        host = both[:, :rows].cpu().numpy()
        return host[0].view(np.uint64), host[1].view(self._dtype)

    def rerank(self, queries, candidates, indices, device: Optional[DeviceScope] = None, out=None):
        """Exact scores of the candidates `indices` lists per query (`szs_rocm_rerank_*`): `scores[q, r]` is the score of
        `queries[q]` and `candidates[indices[q, r]]`, the cell the matrix call would hold there.  `indices` is a `(rows, k)` matrix
        of 8-byte cells with contiguous rows - a NumPy array or a torch tensor, host or device - such as the one `top_k` or
        `Fingerprints.top_k` returns; 2**64 - 1 marks an empty slot (score 0), any other index beyond the candidates is refused.
        `candidates` None: the indices refer to `queries`.  Returns an engine-dtype `(rows, k)` NumPy matrix, or fills `out` (a
        NumPy array or torch tensor of 8-byte cells that shares the row stride of `indices`)."""
        import torch

        queries = _as_strs(queries)
        candidates = None if candidates is None else _as_strs(candidates)
        indices_pointer, stride, (rows, k) = _listed_cells(indices, "indices", None)
        if rows != len(queries):
            raise ValueError(f"`indices` must have one row per query: {rows} rows, {len(queries)} queries")
        if out is not None:
            (scores_pointer,), _ = _cells_of_one_stride((("out", out),), (rows, k), stride)
        scope, gpu_device = _where(self, device)
        _on_call_gpu((("indices", indices), ("out", out)), gpu_device)
        queries, candidates = _same_flavour(queries, candidates)
        if out is None:
            if stride == k:
                results = torch.empty((max(rows, 1), k), dtype=torch.int64, device=torch.device("cuda", gpu_device))
            else:  # the scores share the stride of the indices: a host matrix as wide as theirs
                results = np.zeros((max(rows, 1), stride), dtype=np.int64)
            scores_pointer = results.data_ptr() if stride == k else results.ctypes.data
        _tape_call("szs_rocm_rerank", scope, self.handle, queries, candidates, gpu_device, indices_pointer, k, scores_pointer, stride)
        if out is not None:
            return out
        host = results[:rows].cpu().numpy() if stride == k else results[:rows, :k]
        return host.view(self._dtype)

    def fuzzy_find(self, queries, candidates, indices=None, device: Optional[DeviceScope] = None, out=None, starts=False):
        """The best match of every query INSIDE the candidates listed for it (`szs_rocm_fuzzy_find_*`): returns `(distances, ends)`,
        two `uint64` `(rows, k)` NumPy matrices - `distances[q, r]` is the fewest edits that turn `queries[q]` into some substring of
        `candidates[indices[q, r]]`, `ends[q, r]` the smallest exclusive byte offset at which such a substring ends (0: the empty one).
        `indices` is what `rerank` takes; None is the dense form, every query in every candidate: the results are
        `(rows, len(candidates))`.  `candidates` None: the indices refer to `queries` (and must be given).  2**64 - 1 marks an empty
        slot (0, 0).  `out`: a pair of NumPy arrays or torch tensors of 8-byte cells that share the row stride of `indices`, filled
        and returned.  Unit-cost byte Levenshtein engines only, queries of at most 256 bytes.
        `starts=True` (`szs_rocm_fuzzy_find_spans_*`): returns `(distances, starts, ends)` - `candidates[i][starts[q, r]:ends[q, r]]`
        is the shortest best match that ends at `ends[q, r]` - and `out` is a triple in that order."""
        import torch

        names = ("distances", "starts", "ends") if starts else ("distances", "ends")
        queries = _as_strs(queries)
        candidates = None if candidates is None else _as_strs(candidates)
        rows, named = len(queries), ()
        if indices is None:
            if candidates is None or len(candidates) < 1:
                raise ValueError("`indices` None needs at least one candidate; `candidates` None needs `indices`")
            indices_pointer, k, stride = None, len(candidates), None
        else:
            indices_pointer, stride, (index_rows, k) = _listed_cells(indices, "indices", None)
            if index_rows != rows:
                raise ValueError(f"`indices` must have one row per query: {index_rows} rows, {rows} queries")
        if out is not None:
            named = _named_out(out, names)
            output_pointers, stride = _cells_of_one_stride(named, (rows, k), stride)
        scope, gpu_device = _where(self, device)
        _on_call_gpu((("indices", indices),) + named, gpu_device)
        queries, candidates = _same_flavour(queries, candidates)
        if out is None:
            if stride is None or stride == k:
                stride = k
                results = torch.empty((len(names), max(rows, 1), k), dtype=torch.int64, device=torch.device("cuda", gpu_device))
                output_pointers = [matrix.data_ptr() for matrix in results]
            else:  # the outputs share the stride of the indices: host matrices as wide as theirs
                results = np.zeros((len(names), max(rows, 1), stride), dtype=np.int64)
                output_pointers = [matrix.ctypes.data for matrix in results]
        _tape_call("szs_rocm_fuzzy_find_spans" if starts else "szs_rocm_fuzzy_find", scope, self.handle, queries, candidates, gpu_device,
                   indices_pointer, k, *output_pointers, stride)
        if out is not None:
            return out
        host = results[:, :rows].cpu().numpy() if isinstance(results, torch.Tensor) else results[:, :rows, :k]
        return tuple(matrix.view(np.uint64) for matrix in host)

    def align(self, queries, candidates, indices=None, starts=None, ends=None, capacity=None, device: Optional[DeviceScope] = None,
              out=None):
        """WHICH edits (`szs_rocm_alignments_*`): returns `(distances, lengths, ops)` - two `uint64` `(rows, k)` NumPy matrices and a
        `uint8` `(rows, k, capacity)` array.  Slot `(q, r)` pairs `queries[q]` with `c = candidates[indices[q, r]]`, or with
        `c[starts[q, r]:ends[q, r]]` where `starts` and `ends` are given (both or neither: what `fuzzy_find(..., starts=True)` and
        `fuzzy_scan_occurrences` return): `distances` is their Levenshtein distance, `lengths` the number `L` of ops of the canonical
        edit script, `ops[q, r, :L]` that script in forward order as the bytes `= X I D` (extended CIGAR, the query as the read; 'I'
        is a byte of the query alone, 'D' one of the candidate alone) and zeros behind it.  A script of more than `capacity` ops keeps
        its `L` and leaves its slot all zero.  `capacity` None: the longest query plus min(512, the longest candidate), which every
        script fits - or, with `out`, what its `ops` holds; 0: distances and lengths only, `ops` comes back None.
        `indices` and `candidates` None are `fuzzy_find`'s; an index of 2**64 - 1 or a span of (2**64 - 1, 2**64 - 1) is an empty slot
        (0, 0, zeros).  `out`: a triple of NumPy arrays or torch tensors - the two matrices of 8-byte cells share the row stride of
        `indices`, `ops` is contiguous in its last two dimensions with the same row stride in slots - filled and returned.
        Unit-cost byte Levenshtein engines only, queries of at most 256 bytes, spans (or whole candidates) of at most 512."""
        import torch

        queries = _as_strs(queries)
        candidates = None if candidates is None else _as_strs(candidates)
        rows = len(queries)
        if (starts is None) != (ends is None):
            raise ValueError("`starts` and `ends` must both be given, or neither")
        stride, k = None, None
        if indices is None and (candidates is None or len(candidates) < 1):
            raise ValueError("`indices` None needs at least one candidate; `candidates` None needs `indices`")
        if indices is None:
            k = len(candidates)
        input_pointers = []
        for matrix, name in ((indices, "indices"), (starts, "starts"), (ends, "ends")):
            if matrix is None:
                input_pointers.append(None)
                continue
            pointer, own_stride, shape = _listed_cells(matrix, name, None if k is None else (rows, k))
            if shape[0] != rows:
                raise ValueError(f"`{name}` must have one row per query: {shape[0]} rows, {rows} queries")
            if stride is not None and own_stride != stride:
                raise ValueError("`indices`, `starts` and `ends` must share one row stride")
            stride, k = own_stride, shape[1]
            input_pointers.append(pointer)
        capacity = None if capacity is None else _integer(capacity, "capacity", 0)
        named = ()
        if out is not None:
            named = _named_out(out, ("distances", "lengths", "ops"))
            output_pointers, stride = _cells_of_one_stride(named[:2], (rows, k), stride)
            ops = out[2]
            if ops is None:
                if capacity:
                    raise ValueError("`out` ops must not be None when the capacity is not zero")
                capacity, ops_pointer = 0, None
            else:
                shape, itemsize, strides, ops_pointer, _ = _array_facts(ops, "out ops")  # (bytes: the strides count them)
                if capacity is None and len(shape) == 3:
                    capacity = shape[2]
                if len(shape) != 3 or shape != (rows, k, capacity) or itemsize != 1 or capacity < 1 or (
                        capacity > 1 and strides[2] != 1) or (k > 1 and strides[1] != capacity) or (rows > 1 and strides[0] != stride * capacity):
                    raise ValueError("`out` ops must be a (rows, k, capacity) array of bytes, contiguous in its last two dimensions, "
                                     "that shares the row stride of the matrices")
        if capacity is None:
            pool = queries if candidates is None else candidates
            longest = lambda strs: int(np.diff(strs.offsets.astype(np.int64)).max()) if len(strs) else 0  # noqa: E731
            capacity = longest(queries) + min(512, longest(pool))
        scope, gpu_device = _where(self, device)
        _on_call_gpu((("indices", indices), ("starts", starts), ("ends", ends)) + named, gpu_device)
        queries, candidates = _same_flavour(queries, candidates)
        if out is None:
            if stride is None or stride == k:
                stride = k
                cells = torch.empty((2, max(rows, 1), k), dtype=torch.int64, device=torch.device("cuda", gpu_device))
                scripts = torch.empty((max(rows, 1), k, capacity), dtype=torch.uint8, device=torch.device("cuda", gpu_device))
                output_pointers, ops_pointer = [matrix.data_ptr() for matrix in cells], scripts.data_ptr() if capacity else None
            else:  # the outputs share the stride of the inputs: host arrays as wide as theirs
                cells = np.zeros((2, max(rows, 1), stride), dtype=np.int64)
                scripts = np.zeros((max(rows, 1), stride, capacity), dtype=np.uint8)
                output_pointers, ops_pointer = [matrix.ctypes.data for matrix in cells], scripts.ctypes.data if capacity else None
        _tape_call("szs_rocm_alignments", scope, self.handle, queries, candidates, gpu_device, input_pointers[0], k, input_pointers[1],
                   input_pointers[2], *output_pointers, ops_pointer, capacity, stride)
        if out is not None:
            return out
        if isinstance(cells, torch.Tensor):
            cells, scripts = cells[:, :rows].cpu().numpy(), scripts[:rows].cpu().numpy()
        else:
            cells, scripts = cells[:, :rows, :k], scripts[:rows, :k]
        return cells[0].view(np.uint64), cells[1].view(np.uint64), scripts if capacity else None

    def fuzzy_search(self, queries, candidates=None, k=16, device: Optional[DeviceScope] = None, out=None, starts=False):
        """The `k` candidates that contain the best approximate match of every query (`szs_rocm_fuzzy_search_*`): returns
        `(indices, distances, ends)`, three `uint64` `(rows, k)` NumPy matrices - row `q` lists the candidates with the smallest
        `fuzzy_find` distance of `queries[q]`, ascending, ties to the lower index; `distances` and `ends` are what `fuzzy_find` returns
        for those pairs.  `starts=True`: `(indices, distances, starts, ends)`, as `fuzzy_find(..., starts=True)` returns them.
        `candidates` None: self-search, each query's own index excluded.  A row with fewer than `k` candidates ends in index
        2**64 - 1 and zeros.  `out`: a triple - with `starts` a 4-tuple - of NumPy arrays or torch tensors of 8-byte cells in that
        order, of one row stride, filled and returned.  Unit-cost byte Levenshtein engines only, queries of at most 256 bytes."""
        import torch

        k = _integer(k, "k", 1, 1024)
        names = ("indices", "distances", "starts", "ends") if starts else ("indices", "distances", "ends")
        queries = _as_strs(queries)
        candidates = None if candidates is None else _as_strs(candidates)
        rows, named = len(queries), ()
        if out is not None:
            named = _named_out(out, names)
            pointers, stride = _cells_of_one_stride(named, (rows, k))
        scope, gpu_device = _where(self, device)
        _on_call_gpu(named, gpu_device)
        queries, candidates = _same_flavour(queries, candidates)
        if out is None:
            results = torch.empty((len(names), max(rows, 1), k), dtype=torch.int64, device=torch.device("cuda", gpu_device))
            pointers, stride = [matrix.data_ptr() for matrix in results], k
        if not starts:
            pointers = pointers[:2] + [None] + pointers[2:]  # (indices, distances, no starts, ends)
        _tape_call("szs_rocm_fuzzy_search", scope, self.handle, queries, candidates, gpu_device, k, *pointers, stride)
        if out is not None:
            return out
        return tuple(matrix.view(np.uint64) for matrix in results[:, :rows].cpu().numpy())

    def within(self, queries, candidates=None, bound=None, limit=64, device: Optional[DeviceScope] = None, out=None):
        """EVERY candidate of every query inside a score bound (`szs_rocm_within_*`), where `top_k` answers "the k best": returns
        `(counts, indices, scores)` - a `uint64` vector of `len(queries)`, a `uint64` and an engine-dtype `(len(queries), limit)`
        matrix.  A distance engine hits iff `bound >= 0` and `score <= bound`, NW / SW iff the signed `score >= bound`.  `counts[q]`
        is the number of hits among ALL candidates (it may exceed `limit`); `indices[q, i]` and `scores[q, i]` are the `i`-th hit in
        ascending candidate index and its score, and the slots behind hold index 2**64 - 1 and score 0 - the empty slot `rerank`,
        `fuzzy_find` and `align` skip, so the rows feed them directly.  `candidates` None: self-search, each query's own index
        excluded.  `limit=0` counts only: the matrices have shape `(len(queries), 0)`.  `out`: a triple `(counts, indices, scores)`
        of NumPy arrays or torch tensors of 8-byte cells - a contiguous vector and two matrices with contiguous rows of one row
        stride - filled and returned; `scores` may be None, and with `limit=0` so may `indices`.  `limit` at most 65,536."""
        bound = _integer(bound, "bound", -2**63, 2**63 - 1)
        return self._bounded_rows("szs_rocm_within", ("indices", "scores"), ("scores",), queries, candidates, bound, limit, device, out)

    def fuzzy_search_within(self, queries, candidates=None, max_distance=None, limit=64, starts=False, device: Optional[DeviceScope] = None,
                            out=None):
        """EVERY candidate that contains something within `max_distance` edits of the query (`szs_rocm_fuzzy_search_within_*`), where
        `fuzzy_search` answers "the k best": returns `(counts, indices, distances, ends)` - a `uint64` vector of `len(queries)` and
        three `uint64` `(len(queries), limit)` matrices; `starts=True`: `(counts, indices, distances, starts, ends)`.  A hit is a
        candidate whose `fuzzy_find` distance is at most `max_distance` (any non-negative integer below 2**64); `counts[q]` is their
        number among ALL candidates, row `q` lists the leftmost `limit` of them in ascending candidate index, and `distances`, `starts`
        and `ends` are what `fuzzy_find(queries, candidates, indices, starts=...)` returns for those rows, bit for bit.  The slots
        behind hold `(2**64 - 1, 0, 0, 0)`.  A query of no bytes hits every candidate.  `candidates` None: self-search, the own index
        excluded.  `limit=0` counts only.  `out`: a tuple in the order returned, as `within` takes it.  Unit-cost byte Levenshtein
        engines only, queries of at most 256 bytes, `limit` at most 65,536."""
        max_distance = _integer(max_distance, "max_distance", 0, 2**64 - 1)
        names = ("indices", "distances", "starts", "ends") if starts else ("indices", "distances", "ends")
        return self._bounded_rows("szs_rocm_fuzzy_search_within", names, (), queries, candidates, max_distance, limit, device, out)

    def clusters(self, strings, bound, device: Optional[DeviceScope] = None, out=None):
        """The connected components of the graph "i ~ j iff the pair is a `within` hit" (`szs_rocm_clusters_*`): returns
        `(labels, count)` - a `uint64` NumPy vector of `len(strings)` and an `int`.  `hit(i, j)` is `within`'s predicate on the score of
        string `i` against string `j` - a distance engine hits iff `bound >= 0` and `score <= bound`, NW / SW iff the signed
        `score >= bound` - and the graph is undirected: either direction joins the two.  `labels[i]` is the smallest index of the
        component of `i`, so `labels[labels[i]] == labels[i]` and a string with no neighbour labels itself; `count` is the number of
        components.  Nothing truncates - there is no `limit` - and no knob or tile size changes a byte.  `out`: a contiguous NumPy
        vector or torch tensor of `len(strings)` 8-byte cells, host or device, filled and returned in place of `labels`."""
        import torch

        bound = _integer(bound, "bound", -2**63, 2**63 - 1)
        strings = _as_strs(strings)
        rows = len(strings)
        pointer = None if out is None else _vector_cells(out, "out", rows)
        scope, gpu_device = _where(self, device)
        _on_call_gpu((("out", out),), gpu_device)
        if out is None:
            labels = torch.empty(max(rows, 1), dtype=torch.int64, device=torch.device("cuda", gpu_device))
            pointer = labels.data_ptr()
        count = ctypes.c_size_t(0)
        _tape_call("szs_rocm_clusters", scope, self.handle, strings, _ONE_SIDED, gpu_device, bound, pointer, ctypes.byref(count))
        return (labels[:rows].cpu().numpy().view(np.uint64) if out is None else out), int(count.value)

    def _bounded_rows(self, entry, names, optional, queries, candidates, bound, limit, device, out):
        """What `within` and `fuzzy_search_within` share: the checks, a vector of counts and `len(names)` matrices of `limit` slots a
        row behind `entry`'s tape forms (a missing `starts` goes as NULL).  `optional`: the matrices `out` may leave None."""
        import torch

        limit = _integer(limit, "limit", 0, 65536)
        queries = _as_strs(queries)
        candidates = None if candidates is None else _as_strs(candidates)
        rows, named = len(queries), ()
        if out is not None:
            named = _named_out(out, ("counts",) + names)
            counts_pointer = _vector_cells(out[0], "out counts", rows)
            pointers, stride = [], None
            for name, matrix in named[1:]:
                if matrix is None and (name[4:] in optional or not limit):
                    pointers.append(None)
                elif not limit:  # never looked at: only the shape is checked
                    if tuple(getattr(matrix, "shape", ())) != (rows, 0):
                        raise ValueError(f"`{name}` must be None or of shape ({rows}, 0) with limit 0")
                    pointers.append(None)
                else:
                    (pointer,), stride = _cells_of_one_stride(((name, matrix),), (rows, limit), stride)
                    pointers.append(pointer)
            stride = limit if stride is None else stride
        scope, gpu_device = _where(self, device)
        _on_call_gpu(named, gpu_device)
        queries, candidates = _same_flavour(queries, candidates)
        if out is None:
            where = torch.device("cuda", gpu_device)
            results = (torch.empty(max(rows, 1), dtype=torch.int64, device=where),
                       torch.empty((len(names), max(rows, 1), limit), dtype=torch.int64, device=where))
            counts_pointer, stride = results[0].data_ptr(), limit
            pointers = [matrix.data_ptr() if limit else None for matrix in results[1]]
        if entry == "szs_rocm_fuzzy_search_within" and "starts" not in names:
            pointers = pointers[:2] + [None] + pointers[2:]  # (indices, distances, no starts, ends)
        _tape_call(entry, scope, self.handle, queries, candidates, gpu_device, bound, limit, counts_pointer, *pointers, stride)
        if out is not None:
            return out
        counts, matrices = results[0][:rows].cpu().numpy().view(np.uint64), results[1][:, :rows].cpu().numpy()
        return (counts,) + tuple(matrix.view(self._dtype if name == "scores" else np.uint64) for matrix, name in zip(matrices, names))

    def fuzzy_scan(self, queries, text, device: Optional[DeviceScope] = None, out=None, starts=False):
        """The best match of every query inside ONE long text (`szs_rocm_fuzzy_scan_*`): returns `(distances, ends)`, two `uint64`
        NumPy vectors of `len(queries)` - exactly column 0 of `fuzzy_find(queries, [text])`, with the text cut over the device's lanes
        instead of walked on one.  `text` is bytes-like, a NumPy `uint8` array or a torch `uint8` tensor: a tensor on the call's GPU
        goes as a raw pointer, host data is uploaded once.  `starts=True` (`szs_rocm_fuzzy_scan_spans_*`): returns
        `(distances, starts, ends)` - `text[starts[q]:ends[q]]` is the shortest best match that ends at `ends[q]`.  `out`: a pair -
        with `starts` a triple - of contiguous NumPy vectors or torch tensors of `len(queries)` 8-byte cells in that order, filled
        and returned.  Unit-cost byte Levenshtein engines only, queries of at most 256 bytes, a text below 4 GiB."""
        import torch

        names = ("distances", "starts", "ends") if starts else ("distances", "ends")
        queries = _as_strs(queries)
        rows, named = len(queries), ()
        text = _text_bytes(text)
        if out is not None:
            named = _named_out(out, names)
            pointers = [_vector_cells(vector, name, rows) for name, vector in named]
        scope, gpu_device = _where(self, device)
        _on_call_gpu((("text", text),) + named, gpu_device)
        text = _text_on_gpu(text, gpu_device)
        if out is None:
            results = torch.empty((len(names), max(rows, 1)), dtype=torch.int64, device=torch.device("cuda", gpu_device))
            pointers = [vector.data_ptr() for vector in results]
        _tape_call("szs_rocm_fuzzy_scan_spans" if starts else "szs_rocm_fuzzy_scan", scope, self.handle, queries, _ONE_SIDED, gpu_device,
                   text.data_ptr() if text.numel() else None, text.numel(), *pointers)
        if out is not None:
            return out
        return tuple(vector.view(np.uint64) for vector in results[:, :rows].cpu().numpy())

    def fuzzy_scan_matches(self, queries, text, max_distance, limit=64, device: Optional[DeviceScope] = None, out=None):
        """EVERY end within `max_distance` edits of every query inside ONE long text (`szs_rocm_fuzzy_scan_matches_*`): returns
        `(counts, distances, ends)` - a `uint64` vector of `len(queries)` and two `uint64` `(len(queries), limit)` arrays.  A hit of
        `queries[q]` is an exclusive byte offset `j` in `[1, len(text)]` at which some substring of `text` ends that `max_distance` or
        fewer edits turn into the query; `counts[q]` is their number in the whole text (it may exceed `limit`), `ends[q, i]` and
        `distances[q, i]` the `i`-th of them in ascending `j` and its distance, and the slots behind hold 2**64 - 1.  `limit=0`
        counts only: the two arrays have shape `(len(queries), 0)`.  `text` is what `fuzzy_scan` takes.  `out`: a triple of
        contiguous NumPy arrays or torch tensors of 8-byte cells of those shapes, filled and returned.  Unit-cost byte Levenshtein
        engines only, queries of at most 256 bytes, a text below 4 GiB, `limit` at most 2**24."""
        return self._fuzzy_scan_columns("szs_rocm_fuzzy_scan_matches", ("counts", "distances", "ends"), queries, text, max_distance, limit,
                                        device, out)

    def fuzzy_scan_occurrences(self, queries, text, max_distance, limit=64, starts=True, device: Optional[DeviceScope] = None, out=None):
        """ONE span per occurrence of every query inside ONE long text (`szs_rocm_fuzzy_scan_occurrences_*`): returns
        `(counts, distances, starts, ends)` - a `uint64` vector of `len(queries)` and three `uint64` `(len(queries), limit)` arrays;
        `starts=False` returns `(counts, distances, ends)` and launches no reverse pass.  With `D[j]` the fewest edits between
        `queries[q]` and a substring of `text` that ends at byte offset `j` (`D[0]` = the query's length), `j` in `[1, len(text)]` is
        an occurrence end iff `D[j] <= max_distance`, `D[j] < D[j - 1]` and `j == len(text) or D[j] <= D[j + 1]`: the first column of a
        valley floor - one per cluster of `fuzzy_scan_matches` hits, the leftmost of a plateau.  `counts[q]` is their number in the whole
        text (it may exceed `limit`); `ends[q, i]`, `distances[q, i]` and `starts[q, i]` describe the `i`-th of them in ascending
        `j`: `text[starts[q, i]:ends[q, i]]` is the shortest substring ending there at that distance.  Spans of different occurrences
        may overlap.  The slots behind hold 2**64 - 1; `limit=0` counts only: the arrays have shape `(len(queries), 0)`.  `text`,
        `out` (here a quadruple, or a triple with `starts=False`) and the limits are `fuzzy_scan_matches`'."""
        names = ("counts", "distances", "starts", "ends") if starts else ("counts", "distances", "ends")
        return self._fuzzy_scan_columns("szs_rocm_fuzzy_scan_occurrences", names, queries, text, max_distance, limit, device, out)

    def _fuzzy_scan_columns(self, entry, names, queries, text, max_distance, limit, device, out):
        """What `fuzzy_scan_matches` and `fuzzy_scan_occurrences` share: the checks, the text on the device, a vector of counts and
        `len(names) - 1` matrices of `limit` slots a row behind `entry`'s tape forms (a missing `starts` goes as NULL)."""
        import torch

        max_distance, limit = _integer(max_distance, "max_distance", 0, 2**64 - 1), _integer(limit, "limit", 0, 2**24)
        queries = _as_strs(queries)
        rows, named = len(queries), ()
        text = _text_bytes(text)
        if out is not None:
            named = _named_out(out, names)
            pointers = [_vector_cells(out[0], "out counts", rows)]
            for name, matrix in named[1:]:  # the C entries take no row stride: the matrices are contiguous as a whole
                shape, itemsize, strides, pointer, _ = _array_facts(matrix, name)
                dense = 0 in shape or all(extent == 1 or stride == step for extent, stride, step in zip(shape, strides, (limit * 8, 8)))
                if shape != (rows, limit) or itemsize != 8 or not dense:
                    raise ValueError(f"`{name}` must be a contiguous array of shape {(rows, limit)} of 8-byte cells")
                pointers.append(pointer if limit else None)  # limit 0: the matrices are never looked at
        scope, gpu_device = _where(self, device)
        _on_call_gpu((("text", text),) + named, gpu_device)
        text = _text_on_gpu(text, gpu_device)
        if out is None:
            where = torch.device("cuda", gpu_device)
            results = (torch.empty(max(rows, 1), dtype=torch.int64, device=where),
                       torch.empty((len(names) - 1, max(rows, 1), limit), dtype=torch.int64, device=where))
            pointers = [results[0].data_ptr()] + [matrix.data_ptr() if limit else None for matrix in results[1]]
        if entry == "szs_rocm_fuzzy_scan_occurrences" and "starts" not in names:
            pointers = pointers[:2] + [None] + pointers[2:]  # (counts, distances, no starts, ends)
        _tape_call(entry, scope, self.handle, queries, _ONE_SIDED, gpu_device, text.data_ptr() if text.numel() else None, text.numel(),
                   max_distance, limit, *pointers)
        if out is not None:
            return out
        counts, matrices = results[0][:rows].cpu().numpy().view(np.uint64), results[1][:, :rows].cpu().numpy().view(np.uint64)
        return (counts,) + tuple(matrices)

    def __del__(self):
        handle = getattr(self, "handle", None)
        if handle and self._free is not None:
            self._free(handle)
            self.handle = None


class LevenshteinDistances(_Engine):
    """`LevenshteinDistances(match=0, mismatch=1, open=1, extend=1, capabilities=None)` -> uint64 matrix."""

    _free = staticmethod(lib.szs_levenshtein_distances_free)
    _call_u32 = staticmethod(lib.szs_levenshtein_distances_u32tape)
    _call_u64 = staticmethod(lib.szs_levenshtein_distances_u64tape)
    _init = staticmethod(lib.szs_levenshtein_distances_init)
    _dtype = np.uint64

    def __init__(self, match: int = 0, mismatch: int = 1, open: int = 1, extend: int = 1, capabilities=None):
        super().__init__()
        self._remember(capabilities)
        error = ctypes.c_char_p()
        status = self._init(match, mismatch, open, extend, None, self._mask, ctypes.byref(self.handle), ctypes.byref(error))
        _abi.check(status, error)


class LevenshteinDistancesUTF8(LevenshteinDistances):
    """Codepoint-level distances (`szs_levenshtein_distances_utf8*`)."""

    _free = staticmethod(lib.szs_levenshtein_distances_utf8_free)
    _call_u32 = staticmethod(lib.szs_levenshtein_distances_utf8_u32tape)
    _call_u64 = staticmethod(lib.szs_levenshtein_distances_utf8_u64tape)
    _init = staticmethod(lib.szs_levenshtein_distances_utf8_init)


class NeedlemanWunschScores(_Engine):
    """`NeedlemanWunschScores(byte_to_class, class_substitution_costs, open=-1, extend=-1, capabilities=None)`
    -> int64 matrix of global alignment scores (README.md:500-515)."""

    _free = staticmethod(lib.szs_needleman_wunsch_scores_free)
    _call_u32 = staticmethod(lib.szs_needleman_wunsch_scores_u32tape)
    _call_u64 = staticmethod(lib.szs_needleman_wunsch_scores_u64tape)
    _init = staticmethod(lib.szs_needleman_wunsch_scores_init)
    _dtype = np.int64

    def __init__(self, byte_to_class, class_substitution_costs, open: int = -1, extend: int = -1, capabilities=None):
        super().__init__()
        self._remember(capabilities)
        byte_to_class = np.ascontiguousarray(byte_to_class, dtype=np.uint8)
        costs = np.ascontiguousarray(class_substitution_costs, dtype=np.int8)
        if byte_to_class.size != 256 or costs.size != 32 * 32:
            raise ValueError("byte_to_class must hold 256 bytes and class_substitution_costs 32x32 int8 values")
        error = ctypes.c_char_p()
        status = self._init(byte_to_class.ctypes.data, costs.ctypes.data, open, extend, None, self._mask,
                            ctypes.byref(self.handle), ctypes.byref(error))
        _abi.check(status, error)


class SmithWatermanScores(NeedlemanWunschScores):
    """Same arguments, local alignment scores (`szs_smith_waterman_scores*`)."""

    _free = staticmethod(lib.szs_smith_waterman_scores_free)
    _call_u32 = staticmethod(lib.szs_smith_waterman_scores_u32tape)
    _call_u64 = staticmethod(lib.szs_smith_waterman_scores_u64tape)
    _init = staticmethod(lib.szs_smith_waterman_scores_init)


_NO_ROWS = np.zeros(4, dtype=np.uint32)  # where a hash matrix of zero rows points: never NULL, never read


class Fingerprints:
    """`Fingerprints(ndim, window_widths=None, alphabet_size=256, seed=0, capabilities=None)` - rolling MinHash /
    Count-Min sketches (`szs_fingerprints_*`; /root/reference/python/README.md:549-590).  Called as
    `engine(texts, device=None, out=None)`, returns `(hashes, counts)`: two `uint32` matrices of shape `(len(texts), ndim)`."""

    def __init__(self, ndim: int, window_widths=None, alphabet_size: int = 256, seed: int = 0, capabilities=None):
        self.handle = ctypes.c_void_p()
        self.ndim = int(ndim)
        self._scope = capabilities if isinstance(capabilities, DeviceScope) else None
        self._mask = _capability_mask(capabilities)
        widths = None if window_widths is None else np.ascontiguousarray(window_widths, dtype=np.uint64)
        error = ctypes.c_char_p()
        status = lib.szs_fingerprints_init(self.ndim, alphabet_size, None if widths is None else widths.ctypes.data,
                                           0 if widths is None else len(widths), seed, None, self._mask,
                                           ctypes.byref(self.handle), ctypes.byref(error))
        _abi.check(status, error)

    @property
    def capabilities(self) -> tuple:  # the reference spells this one without underscores (README.md:571)
        return _capability_names(self._mask & lib.szs_capabilities())

    def __call__(self, texts, device: Optional[DeviceScope] = None, out=None):
        import torch

        scope = device or self._scope or _get_default_scope()
        gpu_device = scope.gpu_device if scope.gpu_device is not None else 0
        texts = _as_strs(texts)
        rows = len(texts)
        if out is not None:
            hashes, counts = out
            for matrix in (hashes, counts):
                if not isinstance(matrix, np.ndarray) or matrix.shape != (rows, self.ndim) or matrix.dtype != np.uint32 or (
                        rows and matrix.strides[1] != 4):
                    raise ValueError("`out` must be a pair of (len(texts), ndim) uint32 NumPy matrices with contiguous rows")
            pointers = (hashes.ctypes.data, hashes.strides[0] if rows else self.ndim * 4,
                        counts.ctypes.data, counts.strides[0] if rows else self.ndim * 4)
            device_out = None
        else:
            device_out = torch.empty((2, max(rows, 1), self.ndim), dtype=torch.int32, device=torch.device("cuda", gpu_device))
            pointers = (device_out[0].data_ptr(), self.ndim * 4, device_out[1].data_ptr(), self.ndim * 4)
        tape = texts._tape(gpu_device)
        call = lib.szs_fingerprints_u64tape if texts.wide_offsets else lib.szs_fingerprints_u32tape
        error = ctypes.c_char_p()
        _abi.check(call(self.handle, scope.handle, ctypes.byref(tape), pointers[0], pointers[1], pointers[2], pointers[3],
                        ctypes.byref(error)), error)
        if out is not None:
            return out
        both = device_out[:, :rows].cpu().numpy().view(np.uint32)
        return both[0], both[1]

    def _hashes(self, matrix, name):
        """-> (pointer, row stride in bytes, rows, what `_on_call_gpu` looks at) of an `(n, ndim)` matrix of 32-bit hashes with
        contiguous rows: a `uint32` NumPy array, or an `int32` / `uint32` torch tensor on the host or on a GPU (passed by pointer)."""
        ndim = self.ndim
        shape, _, strides, pointer, _ = _array_facts(matrix, name)
        if len(shape) != 2 or shape[1] != ndim or str(matrix.dtype) not in ("uint32", "torch.int32", "torch.uint32"):
            raise ValueError(f"`{name}` must be an (n, {ndim}) matrix of uint32 (a tensor: int32 / uint32) hashes")
        rows = shape[0]  # (the strides of an empty or one-row matrix say nothing)
        if rows and (strides[1] != 4 or (rows > 1 and (strides[0] < ndim * 4 or strides[0] % 4))):
            raise ValueError(f"`{name}` must have contiguous rows")
        if not rows:  # torch gives an empty tensor the pointer 0, and a NULL candidate matrix means self-search to the library
            return _NO_ROWS.ctypes.data, ndim * 4, 0, None
        return pointer, strides[0] if rows > 1 else ndim * 4, rows, matrix

    def _search_inputs(self, query_hashes, candidate_hashes):
        queries = self._hashes(query_hashes, "query_hashes")
        candidates = None if candidate_hashes is None else self._hashes(candidate_hashes, "candidate_hashes")
        return queries, candidates, (("query_hashes", queries[3]), ("candidate_hashes", None if candidates is None else candidates[3]))

    def matches(self, query_hashes, candidate_hashes=None, device: Optional[DeviceScope] = None, out=None):
        """Equal dimensions of every (query, candidate) pair of fingerprints (`szs_rocm_fingerprint_matches`): a `(Q, C)` `uint32`
        matrix.  Inputs are the `(n, ndim)` hash matrices this engine returns - `uint32` NumPy arrays, or `int32` / `uint32` torch
        tensors on the host or the GPU (passed by pointer), with contiguous rows.  `candidate_hashes` None: the queries against
        themselves, diagonal included (= `ndim`).  `out`: a `(Q, C)` NumPy array or torch tensor of `int32` / `uint32` cells with
        contiguous rows, filled and returned.  GPU tensors must live on the scope's GPU.  The Jaccard estimate of a pair is
        `matches / ndim`: that division stays the caller's.  Equality is plain: two 0xFFFFFFFF hashes (a text shorter than the window) count as equal."""
        import torch

        queries, candidates, named = self._search_inputs(query_hashes, candidate_hashes)
        rows, columns = queries[2], queries[2] if candidates is None else candidates[2]
        if out is not None:
            shape, _, strides, pointer, _ = _array_facts(out, "out")
            if shape != (rows, columns) or str(out.dtype) not in ("uint32", "int32", "torch.int32", "torch.uint32") or (
                    columns > 1 and strides[1] != 4) or strides[0] % 4:
                raise ValueError("`out` must be a (queries, candidates) matrix of int32 / uint32 cells with contiguous rows")
            stride = strides[0] if rows > 1 else max(columns, 1) * 4
        scope, gpu_device = _where(self, device)
        _on_call_gpu(named + (("out", out),), gpu_device)
        if out is None:
            results = torch.empty((max(rows, 1), max(columns, 1)), dtype=torch.int32, device=torch.device("cuda", gpu_device))
            pointer, stride = results.data_ptr(), max(columns, 1) * 4
        message = ctypes.c_char_p()
        status = lib.szs_rocm_fingerprint_matches(
            self.handle, scope.handle, queries[0], queries[1], rows, None if candidates is None else candidates[0],
            0 if candidates is None else candidates[1], 0 if candidates is None else columns, pointer, stride, ctypes.byref(message))
        _abi.check(status, message)
        if out is not None:
            return out
        return results[:rows, :columns].cpu().numpy().view(np.uint32)

    def top_k(self, query_hashes, candidate_hashes=None, k=None, device: Optional[DeviceScope] = None, out=None):
        """The `k` candidates with the MOST equal dimensions per query (`szs_rocm_fingerprint_top_k`), without the matrix: returns
        `(indices, matches)`, two `uint64` `(Q, k)` NumPy matrices, or fills `out=(indices, matches)` (NumPy arrays or torch
        tensors of 8-byte cells, one row stride; `matches` may be None).  Inputs as for `matches()`.  Ties go to the lower candidate
        index.  `candidate_hashes` None: self-search, each query's own index excluded (identical fingerprints at other indices
        count).  A row with fewer than `k` candidates ends in index 2**64 - 1 and count 0.  The Jaccard estimate of a hit is
        `matches / ndim`: that division stays the caller's."""
        import torch

        k = _integer(k, "k", 1, 1024)
        queries, candidates, named = self._search_inputs(query_hashes, candidate_hashes)
        rows = queries[2]
        if out is not None:
            indices_pointer, matches_pointer, stride, named_out = _top_k_out(out, "matches", (rows, k))
            named += named_out
        scope, gpu_device = _where(self, device)
        _on_call_gpu(named, gpu_device)
        if out is None:
            both = torch.empty((2, max(rows, 1), k), dtype=torch.int64, device=torch.device("cuda", gpu_device))
            indices_pointer, matches_pointer, stride = both[0].data_ptr(), both[1].data_ptr(), k
        message = ctypes.c_char_p()
        status = lib.szs_rocm_fingerprint_top_k(
            self.handle, scope.handle, queries[0], queries[1], rows, None if candidates is None else candidates[0],
            0 if candidates is None else candidates[1], 0 if candidates is None else candidates[2], k, indices_pointer,
            matches_pointer, stride, ctypes.byref(message))
        _abi.check(status, message)
        if out is not None:
            return out
        host = both[:, :rows].cpu().numpy().view(np.uint64)
        return host[0], host[1]

    def clusters(self, hashes, min_matches, device: Optional[DeviceScope] = None, out=None):
        """The connected components of "rows `i` and `j` share at least `min_matches` equal dimensions"
        (`szs_rocm_fingerprint_clusters`): returns `(labels, count)` as the similarity engines' `clusters` does - `labels[i]` the
        smallest row of the component of row `i`, a `uint64` NumPy vector, and the number of components.  `hashes` as `top_k` takes
        them.  `min_matches=0` makes every pair a hit - one cluster; beyond `ndim` none.  `out`: a contiguous NumPy vector or torch
        tensor of 8-byte cells, host or device, filled and returned in place of `labels`."""
        import torch

        min_matches = _integer(min_matches, "min_matches", 0, 2**64 - 1)
        side = self._hashes(hashes, "hashes")
        rows = side[2]
        pointer = None if out is None else _vector_cells(out, "out", rows)
        scope, gpu_device = _where(self, device)
        _on_call_gpu((("hashes", side[3]), ("out", out)), gpu_device)
        if out is None:
            labels = torch.empty(max(rows, 1), dtype=torch.int64, device=torch.device("cuda", gpu_device))
            pointer = labels.data_ptr()
        message, count = ctypes.c_char_p(), ctypes.c_size_t(0)
        status = lib.szs_rocm_fingerprint_clusters(self.handle, scope.handle, side[0], side[1], rows, min_matches, pointer,
                                                   ctypes.byref(count), ctypes.byref(message))
        _abi.check(status, message)
        return (labels[:rows].cpu().numpy().view(np.uint64) if out is None else out), int(count.value)

    def __del__(self):
        handle = getattr(self, "handle", None)
        if handle and lib is not None:
            lib.szs_fingerprints_free(handle)
            self.handle = None


class NodeEngine:
    """One cost model on every GPU of a `Node`; `engine(queries, candidates=None, out=None)` scores the whole cross-product
    with its query rows dealt over the GPUs (`szs_rocm_node_scores_*`, csrc/host/node.c) and returns the per-GPU statistics
    of the call as a dict (the matrix lands in `out`, or is returned when `out` is None)."""

    def __init__(self, node: "Node", kind: str, *arguments):
        self.node = node
        self.handle = ctypes.c_void_p()
        error = ctypes.c_char_p()
        init = getattr(lib, f"szs_rocm_node_{kind}_init")
        if kind in ("needleman_wunsch_scores", "smith_waterman_scores"):
            byte_to_class = np.ascontiguousarray(arguments[0], dtype=np.uint8)
            costs = np.ascontiguousarray(arguments[1], dtype=np.int8)
            if byte_to_class.size != 256 or costs.size != 32 * 32:
                raise ValueError("byte_to_class must hold 256 bytes and class_substitution_costs 32x32 int8 values")
            status = init(node.handle, byte_to_class.ctypes.data, costs.ctypes.data, arguments[2], arguments[3],
                          ctypes.byref(self.handle), ctypes.byref(error))
        else:
            status = init(node.handle, *arguments, ctypes.byref(self.handle), ctypes.byref(error))
        _abi.check(status, error)
        self._signed = kind in ("needleman_wunsch_scores", "smith_waterman_scores")
        self.last_stats: Optional[dict] = None

    def __call__(self, queries, candidates=None, out=None):
        import torch

        queries = _as_strs(queries)
        candidates = None if candidates is None else _as_strs(candidates)
        if candidates is not None and queries.wide_offsets != candidates.wide_offsets:
            queries = Strs.from_tape(queries.data, queries.offsets.astype(np.uint64))
            candidates = Strs.from_tape(candidates.data, candidates.offsets.astype(np.uint64))
        rows, columns = len(queries), len(queries if candidates is None else candidates)

        def tape_of(strs):  # where the bytes already are: a GPU if they were moved there, else host memory
            if strs._device is not None and strs._device[0] != "cpu":
                return strs._tape(strs._device[0])
            tape_type = _abi.U64Tape if strs.wide_offsets else _abi.U32Tape
            return tape_type(strs.data.ctypes.data, strs.offsets.ctypes.data, strs.count)

        q_tape = tape_of(queries)
        c_tape = None if candidates is None else tape_of(candidates)
        if out is None:
            results = np.zeros((rows, max(columns, 1)), dtype=np.int64)[:, :columns]
            pointer, stride = results.ctypes.data, max(columns, 1)
        elif isinstance(out, np.ndarray):
            if out.shape != (rows, columns) or out.dtype.itemsize != 8 or (columns and out.strides[1] != 8):
                raise ValueError("`out` must be a (rows, columns) matrix of 8-byte cells with contiguous rows")
            results, pointer, stride = out, out.ctypes.data, out.strides[0] // 8
        else:
            if tuple(out.shape) != (rows, columns) or out.element_size() != 8 or (columns and out.stride(1) != 1):
                raise ValueError("`out` must be a (rows, columns) matrix of 8-byte cells with contiguous rows")
            results, pointer, stride = out, out.data_ptr(), out.stride(0) if rows > 1 else max(columns, 1)
        stats, error = _abi.NodeStats(), ctypes.c_char_p()
        call = lib.szs_rocm_node_scores_u64tape if queries.wide_offsets else lib.szs_rocm_node_scores_u32tape
        status = call(self.handle, ctypes.byref(q_tape), None if c_tape is None else ctypes.byref(c_tape), pointer, stride,
                      ctypes.byref(stats), ctypes.byref(error))
        _abi.check(status, error)
        gpus = int(stats.gpus)
        self.last_stats = {
            "gpus": gpus, "wall_ms": float(stats.wall_milliseconds), "busy_ms": [float(stats.busy_milliseconds[i]) for i in range(gpus)],
            "kernel_ms": [float(stats.kernel_milliseconds[i]) for i in range(gpus)], "cells": [int(stats.cells[i]) for i in range(gpus)],
            "rows": [int(stats.rows[i]) for i in range(gpus)], "row_weights": [int(stats.row_weights[i]) for i in range(gpus)],
            "peer_copies": [int(stats.peer_copies[i]) for i in range(gpus)], "staged_copies": [int(stats.staged_copies[i]) for i in range(gpus)],
            "peer_pairs": int(stats.peer_pairs), "symmetric": bool(stats.symmetric),
        }
        if out is None:
            return results.view(np.int64 if self._signed else np.uint64)
        return self.last_stats

    def __del__(self):
        handle = getattr(self, "handle", None)
        if handle and lib is not None:
            lib.szs_rocm_node_engine_free(handle)
            self.handle = None


class Node:
    """`Node(gpu_devices=None)` - a set of GPUs of this host driven from ONE process, one host thread per GPU inside the
    library (`szs_rocm_node_*`).  The multi-process flavour over `torch.distributed` is `stringzilla_amd.sharded`."""

    def __init__(self, gpu_devices: Optional[Sequence[int]] = None):
        self.handle = ctypes.c_void_p()
        error = ctypes.c_char_p()
        devices = None if gpu_devices is None else np.ascontiguousarray(list(gpu_devices), dtype=np.uint64)
        status = lib.szs_rocm_node_init(None if devices is None else devices.ctypes.data, 0 if devices is None else len(devices),
                                        ctypes.byref(self.handle), ctypes.byref(error))
        _abi.check(status, error)

    def __len__(self) -> int:
        return int(lib.szs_rocm_node_size(self.handle))

    def levenshtein_distances(self, match=0, mismatch=1, open=1, extend=1) -> NodeEngine:
        return NodeEngine(self, "levenshtein_distances", match, mismatch, open, extend)

    def levenshtein_distances_utf8(self, match=0, mismatch=1, open=1, extend=1) -> NodeEngine:
        return NodeEngine(self, "levenshtein_distances_utf8", match, mismatch, open, extend)

    def needleman_wunsch_scores(self, byte_to_class, class_substitution_costs, open=-1, extend=-1) -> NodeEngine:
        return NodeEngine(self, "needleman_wunsch_scores", byte_to_class, class_substitution_costs, open, extend)

    def smith_waterman_scores(self, byte_to_class, class_substitution_costs, open=-1, extend=-1) -> NodeEngine:
        return NodeEngine(self, "smith_waterman_scores", byte_to_class, class_substitution_costs, open, extend)

    def engine_for(self, load) -> NodeEngine:
        """The engine a `workloads.Workload` names."""
        from . import matrices

        if load.kind == "levenshtein":
            return self.levenshtein_distances(**load.costs)
        if load.kind == "levenshtein_utf8":
            return self.levenshtein_distances_utf8(**load.costs)
        make = self.needleman_wunsch_scores if load.kind == "needleman_wunsch" else self.smith_waterman_scores
        return make(*matrices.by_name(load.table), **load.costs)

    def __del__(self):
        handle = getattr(self, "handle", None)
        if handle and lib is not None:
            lib.szs_rocm_node_free(handle)
            self.handle = None
