"""Python interface of cudaextender: ungapped X-drop extension of seed pairs on the GPU (libcudaextender.so, HIP for
gfx950), over the flat C API of include/gw_extender_capi.h.

    ext = UngappedXDropExtender(score_matrix, xdrop_threshold=910, no_entropy=False)
    segments = ext.extend(encode_sequence(query), encode_sequence(target), 3000, seed_pairs)

`seed_pairs` is [N, 2] with columns (target position, query position), the column order of the reference's seed CSV.
numpy inputs go through the host-pointer API; torch tensors on the GPU go through the device-pointer API. The result is
a numpy structured array of SEGMENT records (query, target, length, score), in the library's sorted order."""
import ctypes as C

import numpy as np

from . import _native

# cudaextender::StatusType (cudaextender.hpp)
success = 0
invalid_operation = 1
invalid_input = 2
generic_error = 3
# cudaextender::ExtensionType
ungapped_xdrop = 0

SEGMENT = np.dtype([("query", "<u4"), ("target", "<u4"), ("length", "<i4"), ("score", "<i4")])

# symbol codes of cudaextender/utils.hpp: A C G T, lower-case acgt (L), N/n, other (X), '&' (E)
A_NT, C_NT, G_NT, T_NT, L_NT, N_NT, X_NT, E_NT = range(8)
_CODE = np.full(256, X_NT, np.int8)
for _s, _v in (("A", A_NT), ("C", C_NT), ("G", G_NT), ("T", T_NT), ("N", N_NT), ("n", N_NT), ("&", E_NT)):
    _CODE[ord(_s)] = _v
for _s in "acgt":
    _CODE[ord(_s)] = L_NT


class ExtenderError(RuntimeError):
    def __init__(self, what, status=generic_error):
        super().__init__(what)
        self.status = status


def encode_sequence(seq):
    """str / bytes -> np.int8 codes (encode_sequence of cudaextender/utils.hpp)."""
    b = seq.encode() if isinstance(seq, str) else bytes(seq)
    return _CODE[np.frombuffer(b, np.uint8)]


def _is_gpu_tensor(x):
    return type(x).__module__.startswith("torch") and getattr(x, "is_cuda", False)


def _stream_handle(stream):
    if stream is None:
        return None
    if isinstance(stream, int):
        return stream or None
    for attr in ("cuda_stream", "stream"):  # torch.cuda.Stream, genomeworks_amd.cuda.CudaStream
        if hasattr(stream, attr):
            v = getattr(stream, attr)
            return v() if callable(v) else v
    raise TypeError("stream must be None, an integer handle, a torch.cuda.Stream or a CudaStream")


class UngappedXDropExtender:
    """cudaextender::create_extender(score_matrix, 64, xdrop_threshold, no_entropy, stream, device_id, allocator)."""

    def __init__(self, score_matrix, xdrop_threshold, no_entropy=False, device_id=0, stream=None,
                 max_device_memory=0, extension_type=ungapped_xdrop):
        self._L = _native.extender()
        self._h = None
        m = np.ascontiguousarray(np.asarray(score_matrix, np.int32).reshape(-1))
        self._stream = _stream_handle(stream)
        self.device_id = int(device_id)
        h = self._L.gw_extender_create(m.ctypes.data, m.size, int(xdrop_threshold), int(bool(no_entropy)),
                                       self._stream, self.device_id, int(max_device_memory), int(extension_type))
        if not h:
            raise ExtenderError(self._L.gw_extender_last_error().decode(), invalid_input)
        self._h = h

    def __del__(self):
        if getattr(self, "_h", None):
            self._L.gw_extender_destroy(self._h)
            self._h = None

    def _check(self, rc, what):
        if rc != success:
            msg = self._L.gw_extender_last_error().decode() if rc == -1 else "status %d" % rc
            raise ExtenderError("%s failed: %s" % (what, msg), rc)

    # ---- the Extender methods, one to one ----
    def extend_async_host(self, query, target, score_threshold, seed_pairs_qt):
        """Host-pointer extend_async. seed_pairs_qt: SeedPair records, i.e. [N, 2] uint32 (query, target)."""
        q = np.ascontiguousarray(query, np.int8)
        t = np.ascontiguousarray(target, np.int8)
        s = np.ascontiguousarray(seed_pairs_qt, np.uint32).reshape(-1, 2)
        return self._L.gw_extender_extend_host(self._h, q.ctypes.data, q.size, t.ctypes.data, t.size,
                                               int(score_threshold), s.ctypes.data, len(s))

    def sync(self):
        return self._L.gw_extender_sync(self._h)

    def get_scored_segment_pairs(self):
        n = self._L.gw_extender_result_count(self._h)
        if n < 0:
            raise ExtenderError(self._L.gw_extender_last_error().decode(), invalid_operation)
        out = np.zeros(n, SEGMENT)
        self._check(self._L.gw_extender_copy_results(self._h, out.ctypes.data, n), "get_scored_segment_pairs")
        return out

    def reset(self):
        self._L.gw_extender_reset(self._h)

    def extend_async_device(self, d_query, query_length, d_target, target_length, score_threshold, d_seed_pairs,
                            num_seed_pairs, d_segments, d_count):
        """Device-pointer extend_async on raw device addresses (ints)."""
        return self._L.gw_extender_extend_device(self._h, d_query, int(query_length), d_target, int(target_length),
                                                 int(score_threshold), d_seed_pairs, int(num_seed_pairs), d_segments,
                                                 d_count)

    # ---- convenience ----
    def extend(self, query, target, score_threshold, seed_pairs):
        """Extends seed_pairs ([N, 2] target/query positions) and returns the SEGMENT records. numpy arrays use the
        host-pointer API; GPU torch tensors (query, target int8, seed_pairs integer) use the device-pointer API."""
        if _is_gpu_tensor(query) or _is_gpu_tensor(target) or _is_gpu_tensor(seed_pairs):
            return self._extend_device(query, target, score_threshold, seed_pairs)
        seeds = np.asarray(seed_pairs, np.int64).reshape(-1, 2)
        if seeds.size and (seeds.min() < 0 or seeds.max() > 0xFFFFFFFF):
            raise ExtenderError("seed positions must fit uint32", invalid_input)
        qt = np.ascontiguousarray(seeds[:, ::-1], np.uint32)
        self._check(self.extend_async_host(query, target, score_threshold, qt), "extend_async")
        self._check(self.sync(), "sync")
        return self.get_scored_segment_pairs()

    def _extend_device(self, query, target, score_threshold, seed_pairs):
        import torch
        dev = torch.device("cuda", self.device_id)
        q = torch.as_tensor(query).to(dev, torch.int8).contiguous()
        t = torch.as_tensor(target).to(dev, torch.int8).contiguous()
        s = torch.as_tensor(seed_pairs).to(dev).reshape(-1, 2).flip(1).to(torch.int32).contiguous()  # -> (query, target)
        n = s.shape[0]
        out = torch.empty((max(n, 1), 4), dtype=torch.int32, device=dev)
        count = torch.full((1,), -1, dtype=torch.int32, device=dev)
        # the inputs were made on torch's current stream; the extender runs on its own stream
        torch.cuda.current_stream(dev).synchronize()
        self._check(self.extend_async_device(q.data_ptr(), q.numel(), t.data_ptr(), t.numel(), score_threshold,
                                             s.data_ptr(), n, out.data_ptr(), count.data_ptr()), "extend_async")
        torch.cuda.synchronize(dev)
        k = int(count.item())
        return out[:k].cpu().numpy().view(SEGMENT).reshape(-1).copy()

    # ---- instrumentation / test hooks ----
    def set_chunk_size(self, seeds_per_chunk):
        self._check(self._L.gw_extender_set_chunk_size(self._h, int(seeds_per_chunk)), "set_chunk_size")

    def set_instrumentation(self, enable):
        self._check(self._L.gw_extender_set_instrumentation(self._h, int(bool(enable))), "set_instrumentation")

    def last_timing(self):
        """(kernel_ms, sort_unique_ms, positions) of the last extend call with instrumentation on."""
        k, p, n = C.c_double(), C.c_double(), C.c_int64()
        self._check(self._L.gw_extender_last_timing(self._h, C.byref(k), C.byref(p), C.byref(n)), "last_timing")
        return k.value, p.value, n.value


def sort_unique_device(segments, keep):
    """Test hook: the device compact / sort / de-duplicate step alone (gwx_sort_unique). segments: SEGMENT array (or
    [N, 4] int), keep: [N] bools. Returns the SEGMENT records the step keeps."""
    import torch
    L = _native.extender()
    seg = np.ascontiguousarray(np.asarray(segments).view(np.int32).reshape(-1, 4))
    n = seg.shape[0]
    d_seg = torch.from_numpy(seg.copy()).cuda() if n else torch.zeros((1, 4), dtype=torch.int32, device="cuda")
    d_keep = torch.from_numpy(np.asarray(keep, np.uint8).reshape(-1).copy()).cuda() if n else torch.zeros(1, dtype=torch.uint8, device="cuda")
    d_out = torch.zeros((max(n, 1), 4), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    count = C.c_int32(0)
    rc = L.gw_extender_sort_unique_hook(d_seg.data_ptr(), d_keep.data_ptr(), n, d_out.data_ptr(), C.byref(count), None)
    if rc != 0:
        raise ExtenderError(L.gw_extender_last_error().decode())
    torch.cuda.synchronize()
    return d_out[:count.value].cpu().numpy().view(SEGMENT).reshape(-1).copy()
