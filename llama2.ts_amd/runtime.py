"""Python host layer over the C ABI (include/llama2_hip.h) -- the same seam the N-API binding uses.

It mirrors the reference's names for this path so the parity tests read like the reference:
`readConfig` (llama2.ts:80-93), `readWeights` (:112-129), `newRunState` (:147-163),
`transformer(token, pos, config, state, weights)` (:205-303, call site :468) and `argmax` (:364-366).
Weights and RunState live in HBM; `state.logits` is the only host-visible field, exactly what the
sampling loop (llama2.ts:470-508) consumes.

There is NO CPU fallback: if libllama2hip.so is missing or no gfx950 device is visible every entry
point raises.  (torch is not needed here; the library owns its HIP stream.)
"""
import ctypes as C
import os
import struct

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("L2_LIB_PATH") or os.path.join(_HERE, "lib", "libllama2hip.so")

T_TOKEN_EMBEDDING, T_RMS_ATT, T_WQ, T_WK, T_WV, T_WO, T_RMS_FFN, T_W1, T_W2, T_W3, T_RMS_FINAL, \
    T_FREQ_REAL, T_FREQ_IMAG, T_WCLS = range(14)
TENSOR_NAMES = ["token_embedding_table", "rms_att_weight", "wq", "wk", "wv", "wo", "rms_ffn_weight", "w1", "w2",
                "w3", "rms_final_weight", "freq_cis_real", "freq_cis_imag", "wcls"]
S_X, S_XB, S_XB2, S_HB, S_HB2, S_Q, S_K, S_V, S_ATT, S_LOGITS, S_KEY_CACHE, S_VALUE_CACHE = range(12)
STATE_IDS = dict(x=S_X, xb=S_XB, xb2=S_XB2, hb=S_HB, hb2=S_HB2, q=S_Q, k=S_K, v=S_V, att=S_ATT, logits=S_LOGITS,
                 key_cache=S_KEY_CACHE, value_cache=S_VALUE_CACHE)
OPT_EXACT_ATTENTION, OPT_USE_GRAPH, OPT_KEEP_STATE, OPT_PACKED_MIB, OPT_WEIGHT_MIB, OPT_SAMPLED_TOKENS, OPT_SAMPLED_SERIAL, OPT_AQL_QUEUE, OPT_PREFILL_F32_MFMA, OPT_CHECK_POS = 1, 2, 3, 4, 5, 6, 7, 8, 9, 10
OPT_SEQS = 11      # read-only: sequences reserved by seq_reserve (0 before it)
OPT_BATCH_SAMPLED_TOKENS, OPT_BATCH_SAMPLED_SERIAL = 12, 13   # read-only: decode_sample_batch's and step_batch's sampled tokens, of those by the serial loop
OPT_ATTN_WO_STREAM = 14   # read-only: 1 when a step of the last forward / decode call ran attention and wo as one launch
F_GQA, F_GENERATE_ROPE = 1, 2     # l2_create_ex flags
TP_SOLO_ID = b"L2-SOLO-SHARD-TIMING"   # l2_create_tp id of a shard-timing context (include/llama2_hip.h: L2_TP_SOLO_ID)

# every symbol include/llama2_hip.h declares (tests check the .so exports them all)
ABI_SYMBOLS = ["l2_abi_version", "l2_device_count", "l2_last_error", "l2_create", "l2_destroy", "l2_tp_unique_id",
               "l2_create_tp", "l2_upload", "l2_synth_fill", "l2_read_tensor", "l2_forward", "l2_logits_host",
               "l2_decode_greedy", "l2_decode_sample", "l2_debug_running_sums", "l2_read_state", "l2_set_option", "l2_get_option", "l2_timer_start",
               "l2_timer_stop", "l2_bench_gemv", "l2_bench_decode", "l2_load_checkpoint", "l2_get_header", "l2_prefill", "l2_bench_dominant_in_situ", "l2_tp_mode", "l2_create_ex", "l2_bench_tokens", "l2_dispatch_reason",
               "l2_seq_reserve", "l2_seq_prefill", "l2_forward_batch", "l2_decode_greedy_batch", "l2_read_seq_cache",
               "l2_decode_sample_batch", "l2_seq_prefill_batch", "l2_step_batch", "l2_seq_score_batch", "l2_step_batch_logprobs",
               "l2_seq_fork", "l2_step_batch_constrained", "l2_step_batch_sampling", "l2_debug_sample_controls"]


class SampleControls(C.Structure):
    """l2_sample_controls of include/llama2_hip.h: seven arrays that follow a call's rows, NULL for "off"."""
    _fields_ = [(name, C.c_void_p) for name in ("hist_count", "hist_ids", "repetition", "presence", "frequency", "sample_top_k", "min_p")]


class L2Error(RuntimeError):
    def __init__(self, code, text):
        super().__init__("libllama2hip: %s (code %d)" % (text, code))
        self.code = code


_lib = None


def lib():
    """Load libllama2hip.so (raises if it was not built: there is no fallback path)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("HIP extension missing: %s (run __graft_entry__.build())" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    vp, i32, u32, sz = C.c_void_p, C.c_int, C.c_uint32, C.c_size_t
    L.l2_abi_version.restype = i32
    L.l2_device_count.restype = i32
    L.l2_last_error.restype = C.c_char_p
    L.l2_create.argtypes = [vp, i32, C.POINTER(vp)]
    L.l2_destroy.argtypes = [vp]
    L.l2_destroy.restype = None
    L.l2_tp_unique_id.argtypes = [vp]
    L.l2_create_tp.argtypes = [vp, i32, i32, i32, vp, C.POINTER(vp)]
    L.l2_upload.argtypes = [vp, i32, i32, vp, sz]
    L.l2_synth_fill.argtypes = [vp, u32]
    L.l2_read_tensor.argtypes = [vp, i32, i32, sz, vp, sz]
    L.l2_forward.argtypes = [vp, i32, i32, vp]
    L.l2_logits_host.argtypes = [vp]
    L.l2_logits_host.restype = vp
    L.l2_decode_greedy.argtypes = [vp, i32, i32, i32, vp]
    L.l2_debug_running_sums.argtypes = [i32, vp, sz, vp]
    L.l2_decode_sample.argtypes = [vp, i32, i32, i32, C.c_double, C.c_double, C.POINTER(C.c_uint64), vp]
    L.l2_read_state.argtypes = [vp, i32, i32, vp, sz]
    L.l2_set_option.argtypes = [vp, i32, i32]
    L.l2_get_option.argtypes = [vp, i32, C.POINTER(i32)]
    L.l2_timer_start.argtypes = [vp]
    L.l2_timer_stop.argtypes = [vp, C.POINTER(C.c_float)]
    L.l2_bench_gemv.argtypes = [vp, i32, i32, i32, C.POINTER(C.c_float)]
    L.l2_bench_decode.argtypes = [vp, i32, i32, i32, C.POINTER(C.c_float)]
    L.l2_load_checkpoint.argtypes = [C.c_char_p, i32, i32, i32, vp, C.POINTER(vp), C.POINTER(C.c_uint64)]
    L.l2_get_header.argtypes = [vp, vp]
    L.l2_prefill.argtypes = [vp, vp, i32, i32, vp]
    L.l2_bench_dominant_in_situ.argtypes = [vp, i32, i32, i32, C.POINTER(C.c_float), C.POINTER(i32)]
    L.l2_tp_mode.argtypes = [vp]
    L.l2_create_ex.argtypes = [vp, i32, u32, C.POINTER(vp)]
    L.l2_tp_mode.restype = i32
    L.l2_bench_tokens.argtypes = [vp, vp, i32]
    L.l2_dispatch_reason.argtypes = [vp]
    L.l2_dispatch_reason.restype = C.c_char_p
    L.l2_seq_reserve.argtypes = [vp, i32]
    L.l2_seq_prefill.argtypes = [vp, i32, vp, i32, i32, vp]
    L.l2_forward_batch.argtypes = [vp, i32, vp, vp, vp, vp]
    L.l2_decode_greedy_batch.argtypes = [vp, i32, vp, vp, vp, i32, vp]
    L.l2_read_seq_cache.argtypes = [vp, i32, i32, i32, vp, sz]
    L.l2_decode_sample_batch.argtypes = [vp, i32, vp, vp, vp, i32, vp, vp, vp, vp]
    L.l2_seq_prefill_batch.argtypes = [vp, i32, vp, vp, vp, vp, vp]
    L.l2_step_batch.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.l2_seq_score_batch.argtypes = [vp, i32, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp]
    L.l2_step_batch_logprobs.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp]
    L.l2_seq_fork.argtypes = [vp, i32, i32, vp, i32]
    L.l2_step_batch_constrained.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, i32, vp, vp, vp, vp]
    L.l2_step_batch_sampling.argtypes = L.l2_step_batch_constrained.argtypes + [C.POINTER(SampleControls)]
    L.l2_debug_sample_controls.argtypes = [i32, i32, i32, vp, vp, C.POINTER(SampleControls), vp, vp]
    for name in ABI_SYMBOLS:   # fail at load time, not at first use, if the .so is stale
        getattr(L, name)
    _lib = L
    return L


def _check(rc):
    if rc != 0:
        raise L2Error(rc, lib().l2_last_error().decode("utf8", "replace"))


class Config:
    """`Config` of the reference (llama2.ts:69-79)."""

    def __init__(self, hdr):
        hdr = tuple(int(v) for v in hdr)
        assert len(hdr) == 7
        self.header = hdr
        (self.dim, self.hidden_dim, self.n_layers, self.n_heads, self.n_kv_heads, vocab, self.seq_len) = hdr
        self.vocab_size = abs(vocab)
        self.shared_weights = vocab > 0
        self.head_size = self.dim // self.n_heads


def pack_mask(allowed, V):
    """A token mask of l2_step_batch_constrained as uint32[ceil(V / 32)]: token j is bit j & 31 of word j >> 5.  `allowed`: an iterable
    of ids in [0, V), or a bool array of V entries."""
    V = int(V)
    a = np.asarray(allowed if isinstance(allowed, np.ndarray) else list(allowed))
    W = (V + 31) // 32
    bits = np.zeros(32 * W, dtype=bool)
    if a.dtype == np.bool_:
        if a.shape != (V,):
            raise ValueError("a bool mask needs exactly vocab_size = %d entries" % V)
        bits[:V] = a
    elif a.size:
        if a.dtype.kind not in "iu":
            raise ValueError("token ids must be integers")
        ids = a.reshape(-1).astype(np.int64)
        if ids.min() < 0 or ids.max() >= V:
            raise ValueError("token id outside [0, vocab_size = %d)" % V)
        bits[ids] = True
    return np.packbits(bits, bitorder="little").view("<u4").astype(np.uint32)


def running_sums(values, device=0):
    """S_i = fl(S_{i-1} + values[i]) in fp64, on the device (diagnostic for the sampler's exact parallel accumulation)."""
    v = np.ascontiguousarray(values, dtype=np.float32)
    out = np.empty(v.size, dtype=np.float64)
    _check(lib().l2_debug_running_sums(int(device), v.ctypes.data, v.size, out.ctypes.data))
    return out


def sample_controls(n, history=None, repetition_penalty=None, presence_penalty=None, frequency_penalty=None, top_k=None, min_p=None):
    """The l2_sample_controls of n rows from per-row lists (None, or one entry per row with None for "off"); returns (struct, the
    arrays it points into: keep them alive as long as the struct is used)."""
    def column(vals, dtype, off, what):
        if vals is None:
            return None
        vals = list(vals)
        if len(vals) != n:
            raise ValueError("one %s entry per row" % what)
        return np.array([off if v is None else v for v in vals], dtype=dtype)

    cnt = ids = None
    if history is not None:
        history = list(history)
        if len(history) != n:
            raise ValueError("one history entry per row")
        hs = [np.zeros(0, dtype=np.int32) if h is None else np.ascontiguousarray(h, dtype=np.int32).reshape(-1) for h in history]
        cnt = np.array([h.size for h in hs], dtype=np.int32)
        ids = np.ascontiguousarray(np.concatenate(hs), dtype=np.int32) if n else np.zeros(0, dtype=np.int32)
    cols = [cnt, ids, column(repetition_penalty, np.float64, 1.0, "repetition_penalty"), column(presence_penalty, np.float64, 0.0, "presence_penalty"),
            column(frequency_penalty, np.float64, 0.0, "frequency_penalty"), column(top_k, np.int32, 0, "top_k"), column(min_p, np.float64, 0.0, "min_p")]
    return SampleControls(*[None if a is None or (a is ids and a.size == 0) else a.ctypes.data for a in cols]), cols


def debug_sample_controls(logits, temperature=None, history=None, repetition_penalty=None, presence_penalty=None, frequency_penalty=None,
                          top_k=None, min_p=None, device=0):
    """The penalty and truncation launches of l2_step_batch_sampling on caller-supplied rows, with no model (l2_debug_sample_controls):
    returns (penalised, truncated), each shaped like `logits` (n_rows, vocab).  The keywords are step_batch's."""
    x = np.ascontiguousarray(logits, dtype=np.float32)
    if x.ndim != 2:
        raise ValueError("logits: (n_rows, vocab)")
    n, V = x.shape
    temp = None if temperature is None else np.ascontiguousarray(np.broadcast_to(np.asarray(temperature, dtype=np.float64), (n,)))
    sc, keep = sample_controls(n, history, repetition_penalty, presence_penalty, frequency_penalty, top_k, min_p)
    pen, tr = np.empty_like(x), np.empty_like(x)
    _check(lib().l2_debug_sample_controls(int(device), n, V, x.ctypes.data, None if temp is None else temp.ctypes.data, C.byref(sc),
                                          pen.ctypes.data, tr.ctypes.data))
    del keep
    return pen, tr


def readConfig(buf):
    """readConfig (llama2.ts:80-93): 7 little-endian int32."""
    return Config(struct.unpack("<7i", bytes(buf[:28])))


def tensor_shapes(cfg, gqa=False):
    """[(kind, n_layers_or_0, per-array float count)] in checkpoint order (llama2.ts:114-127).  `gqa`: wk / wv have
    n_kv_heads * head_size rows (contexts created with F_GQA); the reference always reads (d, d)."""
    d, h, L, V, S, hs2 = cfg.dim, cfg.hidden_dim, cfg.n_layers, cfg.vocab_size, cfg.seq_len, cfg.head_size // 2
    kvd = cfg.n_kv_heads * cfg.head_size if gqa else d
    out = [(T_TOKEN_EMBEDDING, 0, V * d), (T_RMS_ATT, L, d), (T_WQ, L, d * d), (T_WK, L, kvd * d), (T_WV, L, kvd * d),
           (T_WO, L, d * d), (T_RMS_FFN, L, d), (T_W1, L, h * d), (T_W2, L, d * h), (T_W3, L, h * d),
           (T_RMS_FINAL, 0, d), (T_FREQ_REAL, 0, S * hs2), (T_FREQ_IMAG, 0, S * hs2)]
    if not cfg.shared_weights:
        out.append((T_WCLS, 0, V * d))
    return out


class Context:
    """One l2_ctx: weights + RunState of one model on one MI355X (or one rank of a TP group)."""

    def __init__(self, cfg, device=0, tp_rank=0, tp_size=1, nccl_id=None, flags=0):
        self.cfg = cfg if isinstance(cfg, Config) else Config(cfg)
        hdr = (C.c_int32 * 7)(*self.cfg.header)
        h = C.c_void_p()
        self.flags = flags
        if flags and tp_size > 1:
            raise ValueError("l2_create_ex flags (F_GQA / F_GENERATE_ROPE) cannot be combined with tp_size > 1: use l2_load_checkpoint for sharded version-1 files")
        if flags:
            _check(lib().l2_create_ex(hdr, device, int(flags), C.byref(h)))
        elif tp_size > 1:
            idbuf = C.create_string_buffer(bytes(nccl_id), 128)
            _check(lib().l2_create_tp(hdr, device, tp_rank, tp_size, idbuf, C.byref(h)))
        else:
            _check(lib().l2_create(hdr, device, C.byref(h)))
        self._h = h
        self.tp_rank, self.tp_size = tp_rank, tp_size
        self._logits_view = None

    def close(self):
        if getattr(self, "_h", None):
            lib().l2_destroy(self._h)     # frees the pinned logits buffer: views handed out by logits_host() die here
            self._h = None
            self._logits_view = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- weights
    def upload(self, kind, layer, arr):
        a = np.ascontiguousarray(arr, dtype=np.float32)
        _check(lib().l2_upload(self._h, kind, layer, a.ctypes.data, a.size))

    def synth_fill(self, seed):
        _check(lib().l2_synth_fill(self._h, int(seed)))

    def read_tensor(self, kind, layer, offset, n):
        out = np.empty(n, dtype=np.float32)
        _check(lib().l2_read_tensor(self._h, kind, layer, offset, out.ctypes.data, n))
        return out

    # -- forward
    def forward(self, token, pos, out=None, view=False):
        """transformer(token, pos, ...) (llama2.ts:468).  Returns the logits as a fresh array; `out` (float32,
        contiguous, >= vocab_size) receives them in place; `view=True` returns the library's pinned buffer itself --
        zero copy, but the NEXT forward / prefill overwrites it and close() frees it (like state.logits in the
        reference, which every transformer() call rewrites)."""
        if out is not None:
            if out.dtype != np.float32 or not out.flags["C_CONTIGUOUS"] or out.size < self.cfg.vocab_size:
                raise ValueError("logits array must be contiguous float32 with at least vocab_size elements")
            _check(lib().l2_forward(self._h, int(token), int(pos), out.ctypes.data))
            return out
        _check(lib().l2_forward(self._h, int(token), int(pos), None))
        return self.logits_host() if view else np.array(self.logits_host(), copy=True)

    def prefill(self, tokens, pos0=0):
        """Feed a run of (prompt) tokens at pos0.. in chunks of up to 64 tokens; returns the logits of the last position."""
        t = np.ascontiguousarray(tokens, dtype=np.int32)
        _check(lib().l2_prefill(self._h, t.ctypes.data, t.size, int(pos0), None))
        return np.array(self.logits_host(), copy=True)

    def logits_host(self):
        """The pinned host buffer l2_forward fills (V floats), as a numpy VIEW: valid until close(), rewritten by
        every forward / prefill."""
        if self._h is None:
            raise L2Error(-4, "context is closed")
        if self._logits_view is None:
            p = lib().l2_logits_host(self._h)
            self._logits_view = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_float)), shape=(self.cfg.vocab_size,))
        return self._logits_view

    def decode_greedy(self, first_token, pos0, steps):
        out = np.zeros(steps, dtype=np.int32)
        _check(lib().l2_decode_greedy(self._h, int(first_token), int(pos0), int(steps), out.ctypes.data))
        return out

    def decode_sample(self, first_token, pos0, steps, temperature, topp, rng_state):
        """The sampled branch of the loop (llama2.ts:480-493) on the device.  `rng_state`: the reference's rng_seed as an
        int; returns (tokens, advanced rng state)."""
        out = np.zeros(steps, dtype=np.int32)
        st = C.c_uint64(int(rng_state))
        _check(lib().l2_decode_sample(self._h, int(first_token), int(pos0), int(steps), float(temperature), float(topp),
                                      C.byref(st), out.ctypes.data))
        return out, int(st.value)

    # -- independent sequences over this context's weights (batched greedy decode)
    def seq_reserve(self, n):
        """Reserve n sequences (1..64): sequence 0 is this context's own cache, 1..n-1 get caches of their own."""
        _check(lib().l2_seq_reserve(self._h, int(n)))

    def seq_prefill(self, seq, tokens, pos0=0):
        """Feed a run of tokens into sequence `seq` at pos0..; returns the logits of the last position."""
        t = np.ascontiguousarray(tokens, dtype=np.int32)
        out = np.empty(self.cfg.vocab_size, dtype=np.float32)
        _check(lib().l2_seq_prefill(self._h, int(seq), t.ctypes.data, t.size, int(pos0), out.ctypes.data))
        return out

    def seq_prefill_batch(self, seqs, prompts, pos0=0):
        """Feed prompts[i] into sequence seqs[i] at pos0[i].. for every i in one packed call; returns the (n, V) logits of every
        prompt's last position.  pos0: a scalar or one per prompt."""
        s = np.ascontiguousarray(seqs, dtype=np.int32).reshape(-1)
        ps = [np.ascontiguousarray(p, dtype=np.int32).reshape(-1) for p in prompts]
        if len(ps) != s.size:
            raise ValueError("one prompt per sequence")
        p0 = np.ascontiguousarray(np.broadcast_to(np.asarray(pos0, dtype=np.int32), (s.size,)))
        nt = np.array([p.size for p in ps], dtype=np.int32)
        tok = np.ascontiguousarray(np.concatenate(ps) if ps else np.zeros(0, dtype=np.int32), dtype=np.int32)
        out = np.empty((s.size, self.cfg.vocab_size), dtype=np.float32)
        _check(lib().l2_seq_prefill_batch(self._h, s.size, s.ctypes.data, nt.ctypes.data, tok.ctypes.data, p0.ctypes.data,
                                          out.ctypes.data))
        return out

    def seq_score_batch(self, seqs, runs, pos0=0, targets=None, top_k=0):
        """Teacher-forced scoring: feed runs[i] into sequence seqs[i] at pos0[i].. exactly as seq_prefill_batch does, and return for
        every fed row, in packed order (the runs back to back): (lp, argmax, top_ids, top_lp) -- the fp64 log-probability of the row's
        target under that position's logits (NaN for a target of -1), the first maximum, and the top_k largest logits' ids / lps
        ((R, top_k) arrays).  targets: R ints in [-1, V), by default each row's next token of its run and -1 at the run's end."""
        s = np.ascontiguousarray(seqs, dtype=np.int32).reshape(-1)
        rs = [np.ascontiguousarray(r, dtype=np.int32).reshape(-1) for r in runs]
        if len(rs) != s.size:
            raise ValueError("one run per sequence")
        p0 = np.ascontiguousarray(np.broadcast_to(np.asarray(pos0, dtype=np.int32), (s.size,)))
        nt = np.array([r.size for r in rs], dtype=np.int32)
        tok = np.ascontiguousarray(np.concatenate(rs) if rs else np.zeros(0, dtype=np.int32), dtype=np.int32)
        if targets is None:
            tg = np.concatenate([np.append(r[1:], -1) for r in rs]).astype(np.int32) if rs else np.zeros(0, dtype=np.int32)
        else:
            tg = np.ascontiguousarray(targets, dtype=np.int32).reshape(-1)
            if tg.size != tok.size:
                raise ValueError("one target per fed row")
        R, k = tok.size, int(top_k)
        lp = np.empty(R, dtype=np.float64)
        am = np.empty(R, dtype=np.int32)
        ids = np.empty((R, max(k, 0)), dtype=np.int32)
        tlp = np.empty((R, max(k, 0)), dtype=np.float64)
        _check(lib().l2_seq_score_batch(self._h, s.size, s.ctypes.data, nt.ctypes.data, tok.ctypes.data, p0.ctypes.data, tg.ctypes.data, k,
                                        lp.ctypes.data, am.ctypes.data, ids.ctypes.data if k > 0 else None,
                                        tlp.ctypes.data if k > 0 else None))
        return lp, am, ids, tlp

    def step_batch(self, seqs, runs, pos0, temperature=0.0, topp=1.0, rng=None, logits=False, logprobs=None, allowed=None, logit_bias=None,
                   history=None, repetition_penalty=None, presence_penalty=None, frequency_penalty=None, top_k=None, min_p=None):
        """One mixed step: feed runs[i] into sequence seqs[i] at pos0[i].. (a run of one token is a decode row), then one pick per row
        from its run's last-position logits, made on the device (temperature 0: argmax, no draw; else one xorshift* draw from rng[i]).
        temperature / topp: a scalar or one per row; rng: one state per row (uint64), or None when every row is greedy.  Returns
        (picks, rng_after[, (n, V) logits the picks were made from]).  logprobs = k (0 .. 20) also returns (pick_lp, top_ids, top_lp):
        each pick's fp64 log-probability under the unscaled logits, and the k largest logits' ids / lps per row ((n, k) arrays).
        allowed: None, or per row None / an iterable of ids / a bool array of V -- the only tokens the row may pick; logit_bias: None,
        or per row None / a {id: value} dict added to those logits (l2_step_batch_constrained: the pick, the returned logits and the
        log-probabilities are all those of the constrained row).  Identical masks are uploaded once.
        history, repetition_penalty, presence_penalty, frequency_penalty, top_k, min_p: None, or per row None for "off" / the row's
        token ids already seen, its penalties on them (applied to the logits before the bias and the mask: visible like those), and
        its sampler-only truncations (l2_step_batch_sampling, called only when one of these is given)."""
        s = np.ascontiguousarray(seqs, dtype=np.int32).reshape(-1)
        n = s.size
        rs = [np.ascontiguousarray(r, dtype=np.int32).reshape(-1) for r in runs]
        if len(rs) != n:
            raise ValueError("one run per sequence")
        p0 = np.ascontiguousarray(np.broadcast_to(np.asarray(pos0, dtype=np.int32), (n,)))
        nt = np.array([r.size for r in rs], dtype=np.int32)
        tok = np.ascontiguousarray(np.concatenate(rs) if rs else np.zeros(0, dtype=np.int32), dtype=np.int32)
        picks = np.zeros(n, dtype=np.int32)
        out = np.empty((n, self.cfg.vocab_size), dtype=np.float32) if logits else None
        temp = np.ascontiguousarray(np.broadcast_to(np.asarray(temperature, dtype=np.float64), (n,)))
        tp = np.ascontiguousarray(np.broadcast_to(np.asarray(topp, dtype=np.float64), (n,)))
        if rng is None:
            if np.any(temp != 0.0):
                raise ValueError("a sampled row needs an rng state")
            st = None
        else:
            st = np.array([int(v) for v in rng], dtype=np.uint64)
            if st.size != n:
                raise ValueError("one rng state per row")
        ptr = lambda a: None if a is None else a.ctypes.data
        controls = (history, repetition_penalty, presence_penalty, frequency_penalty, top_k, min_p)
        with_controls = any(v is not None for v in controls)
        if allowed is not None or logit_bias is not None or with_controls:
            k = 0 if logprobs is None else int(logprobs)
            plp = None if logprobs is None else np.empty(n, dtype=np.float64)
            ids = np.empty((n, max(k, 0)), dtype=np.int32)
            tlp = np.empty((n, max(k, 0)), dtype=np.float64)
            mask_of, masks, bcount, bids, bvals = self._constraints(n, allowed, logit_bias)
            args = (self._h, n, s.ctypes.data, nt.ctypes.data, tok.ctypes.data, p0.ctypes.data,
                    None if st is None else temp.ctypes.data, None if st is None else tp.ctypes.data, ptr(st),
                    picks.ctypes.data, ptr(out), k, ptr(plp), ids.ctypes.data if k > 0 else None,
                    tlp.ctypes.data if k > 0 else None, ptr(mask_of), 0 if masks is None else len(masks),
                    ptr(masks), ptr(bcount), ptr(bids), ptr(bvals))
            if with_controls:
                sc, keep = sample_controls(n, *controls)
                _check(lib().l2_step_batch_sampling(*args, C.byref(sc)))
                del keep
            else:
                _check(lib().l2_step_batch_constrained(*args))
            after = None if st is None else [int(v) for v in st]
            return (picks.tolist(), after) + ((out,) if logits else ()) + (((plp, ids, tlp),) if logprobs is not None else ())
        if logprobs is None:
            _check(lib().l2_step_batch(self._h, n, s.ctypes.data, nt.ctypes.data, tok.ctypes.data, p0.ctypes.data,
                                       None if st is None else temp.ctypes.data, None if st is None else tp.ctypes.data, ptr(st),
                                       picks.ctypes.data, ptr(out)))
            after = None if st is None else [int(v) for v in st]
            return (picks.tolist(), after, out) if logits else (picks.tolist(), after)
        k = int(logprobs)
        plp = np.empty(n, dtype=np.float64)
        ids = np.empty((n, max(k, 0)), dtype=np.int32)
        tlp = np.empty((n, max(k, 0)), dtype=np.float64)
        _check(lib().l2_step_batch_logprobs(self._h, n, s.ctypes.data, nt.ctypes.data, tok.ctypes.data, p0.ctypes.data,
                                            None if st is None else temp.ctypes.data, None if st is None else tp.ctypes.data, ptr(st),
                                            picks.ctypes.data, ptr(out), k, plp.ctypes.data, ids.ctypes.data if k > 0 else None,
                                            tlp.ctypes.data if k > 0 else None))
        after = None if st is None else [int(v) for v in st]
        return (picks.tolist(), after) + ((out,) if logits else ()) + ((plp, ids, tlp),)

    def _constraints(self, n, allowed, logit_bias):
        """The constraint arrays of l2_step_batch_constrained for n rows: (mask_of_row, masks (m, W), bias_count, bias_ids, bias_vals),
        None where the call takes NULL.  Masks are deduplicated by their packed bytes."""
        mask_of = masks = bcount = bids = bvals = None
        if allowed is not None:
            allowed = list(allowed)
            if len(allowed) != n:
                raise ValueError("one allowed entry per row")
            if any(a is not None for a in allowed):
                mask_of = np.full(n, -1, dtype=np.int32)
                seen, packed = {}, []
                for i, a in enumerate(allowed):
                    if a is None:
                        continue
                    m = pack_mask(a, self.cfg.vocab_size)
                    key = m.tobytes()
                    if key not in seen:
                        seen[key] = len(packed)
                        packed.append(m)
                    mask_of[i] = seen[key]
                masks = np.ascontiguousarray(np.stack(packed), dtype=np.uint32)
        if logit_bias is not None:
            logit_bias = list(logit_bias)
            if len(logit_bias) != n:
                raise ValueError("one logit_bias entry per row")
            if any(logit_bias):
                bcount = np.array([len(b) if b else 0 for b in logit_bias], dtype=np.int32)
                bids = np.array([int(t) for b in logit_bias if b for t in b.keys()], dtype=np.int32)
                bvals = np.array([float(v) for b in logit_bias if b for v in b.values()], dtype=np.float32)
        return mask_of, masks, bcount, bids, bvals

    @staticmethod
    def _rows(*cols):
        arrs = [np.ascontiguousarray(c, dtype=np.int32).reshape(-1) for c in cols]
        if len({a.size for a in arrs}) != 1:
            raise ValueError("sequence, token and position lists must have one entry per row")
        return arrs

    def forward_batch(self, seqs, tokens, pos):
        """One transformer() step per row: row i feeds tokens[i] at pos[i] of sequence seqs[i]; returns the (n, V) logits."""
        s, t, p = self._rows(seqs, tokens, pos)
        out = np.empty((s.size, self.cfg.vocab_size), dtype=np.float32)
        _check(lib().l2_forward_batch(self._h, s.size, s.ctypes.data, t.ctypes.data, p.ctypes.data, out.ctypes.data))
        return out

    def decode_greedy_batch(self, seqs, first_tokens, pos0, steps):
        """Device-resident greedy loop over the rows; returns the (n, steps) picked tokens."""
        s, t, p = self._rows(seqs, first_tokens, pos0)
        out = np.zeros((s.size, int(steps)), dtype=np.int32)
        _check(lib().l2_decode_greedy_batch(self._h, s.size, s.ctypes.data, t.ctypes.data, p.ctypes.data, int(steps), out.ctypes.data))
        return out

    def decode_sample_batch(self, seqs, first_tokens, pos0, steps, temperature, topp, rng):
        """Device-resident sampled loop over the rows (llama2.ts:476-493 per row).  temperature / topp: a scalar or one per row; rng: one
        state per row (uint64).  Returns ((n, steps) tokens, [rng state after, per row])."""
        s, t, p = self._rows(seqs, first_tokens, pos0)
        n = s.size
        temp = np.ascontiguousarray(np.broadcast_to(np.asarray(temperature, dtype=np.float64), (n,)))
        tp = np.ascontiguousarray(np.broadcast_to(np.asarray(topp, dtype=np.float64), (n,)))
        st = np.array([int(v) for v in rng], dtype=np.uint64)
        if st.size != n:
            raise ValueError("one rng state per row")
        out = np.zeros((n, int(steps)), dtype=np.int32)
        _check(lib().l2_decode_sample_batch(self._h, n, s.ctypes.data, t.ctypes.data, p.ctypes.data, int(steps), temp.ctypes.data,
                                            tp.ctypes.data, st.ctypes.data, out.ctypes.data))
        return out, [int(v) for v in st]

    def read_seq_cache(self, seq, name, layer=-1):
        """Sequence `seq`'s key_cache / value_cache ([L][S][d] flat, or one layer's [S][d])."""
        c = self.cfg
        n = c.seq_len * c.dim * (c.n_layers if layer < 0 else 1)
        out = np.empty(n, dtype=np.float32)
        _check(lib().l2_read_seq_cache(self._h, int(seq), STATE_IDS[name], int(layer), out.ctypes.data, n))
        return out

    def seq_fork(self, src, dsts, n_pos):
        """Copy cache rows 0 .. n_pos-1 (every layer, keys and values) of sequence `src` into every sequence of `dsts`, in one device
        launch: a sequence that shares its first n_pos tokens with `src` continues at position n_pos.  Blocking."""
        d = np.ascontiguousarray(dsts, dtype=np.int32).reshape(-1)
        _check(lib().l2_seq_fork(self._h, int(src), d.size, d.ctypes.data, int(n_pos)))

    def read_state(self, name, layer=-1):
        c = self.cfg
        dl, hl, Hl = c.dim // self.tp_size, c.hidden_dim // self.tp_size, c.n_heads // self.tp_size
        kvl = (c.n_kv_heads * c.head_size if getattr(self, "flags", 0) & F_GQA else c.dim) // self.tp_size
        slab = c.seq_len * kvl
        n = {"x": c.dim, "xb": dl, "xb2": c.dim, "hb": hl, "hb2": hl, "q": dl, "k": kvl, "v": kvl, "att": Hl * c.seq_len,
             "logits": c.vocab_size, "key_cache": slab * (c.n_layers if layer < 0 else 1),
             "value_cache": slab * (c.n_layers if layer < 0 else 1)}[name]
        out = np.empty(n, dtype=np.float32)
        _check(lib().l2_read_state(self._h, STATE_IDS[name], layer, out.ctypes.data, n))
        return out

    def set_option(self, key, value):
        _check(lib().l2_set_option(self._h, key, int(value)))

    def get_option(self, key):
        v = C.c_int()
        _check(lib().l2_get_option(self._h, key, C.byref(v)))
        return v.value

    def dispatch_reason(self):
        """Why the library's own queue is not in use on this context ("" when it is): l2_dispatch_reason."""
        return lib().l2_dispatch_reason(self._h).decode("utf8", "replace")

    # -- measurement
    def timer_start(self):
        _check(lib().l2_timer_start(self._h))

    def timer_stop(self):
        ms = C.c_float()
        _check(lib().l2_timer_stop(self._h, C.byref(ms)))
        return ms.value

    def bench_gemv(self, kind, layer, iters):
        ms = C.c_float()
        _check(lib().l2_bench_gemv(self._h, kind, layer, iters, C.byref(ms)))
        return ms.value

    def bench_dominant_in_situ(self, first_token, pos0, steps):
        us, n = C.c_float(), C.c_int()
        _check(lib().l2_bench_dominant_in_situ(self._h, first_token, pos0, steps, C.byref(us), C.byref(n)))
        return us.value, n.value

    def tp_mode_id(self):
        return int(lib().l2_tp_mode(self._h))

    def tp_mode(self):
        """How the tensor-parallel step runs (l2_tp_mode): none / RCCL eager / peer-to-peer in a graph / loopback test group."""
        return {0: "single GPU", 1: "eager launches, 2L RCCL fp64 all-reduces + 1 all-gather per token",
                2: "one hipGraph per token with the RCCL collectives captured in it",
                3: "one hipGraph per token, one-shot peer-to-peer fp64 all-reduce inside the residual kernels",
                4: "loopback test group", 5: "shard timing only (one rank alone, exchange against its own inbox)"}.get(lib().l2_tp_mode(self._h), "?")

    def bench_decode(self, first_token, pos0, steps):
        ms = C.c_float()
        _check(lib().l2_bench_decode(self._h, first_token, pos0, steps, C.byref(ms)))
        return ms.value

    def bench_tokens(self, n):
        """The first n tokens the last device-resident run (bench_decode / decode_greedy / decode_sample) chose."""
        out = np.zeros(n, dtype=np.int32)
        _check(lib().l2_bench_tokens(self._h, out.ctypes.data, int(n)))
        return out


class TransformerWeights:
    """Handle to the device-resident TransformerWeights (llama2.ts:95-110)."""

    def __init__(self, ctx):
        self.ctx = ctx


class RunState:
    """RunState (llama2.ts:131-146): only `logits` is host-visible; the rest is read on demand."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.logits = ctx.logits_host()

    def __getattr__(self, name):
        if name in STATE_IDS:
            return self.ctx.read_state(name)
        raise AttributeError(name)


def readWeights(config, f, device=0, ctx=None):
    """readWeights (llama2.ts:112-129): stream each Float32Array of the checkpoint straight to HBM.

    `f` is a binary file object positioned after the 28-byte header.  Each tensor (each layer of a
    per-layer tensor) is read into host memory, uploaded and dropped, so host RAM never holds more
    than one tensor (hard part 5)."""
    ctx = ctx or Context(config, device)
    for kind, layers, count in tensor_shapes(config):
        for layer in range(max(layers, 1)):
            buf = np.frombuffer(f.read(count * 4), dtype="<f4")
            if buf.size != count:
                raise IOError("checkpoint truncated in %s" % TENSOR_NAMES[kind])
            ctx.upload(kind, layer if layers else -1, buf)
    return TransformerWeights(ctx)


def newRunState(config, weights):
    """newRunState (llama2.ts:147-163): the buffers already exist on the device; wrap them."""
    return RunState(weights.ctx)


def transformer(token, pos, config, state, weights):
    """transformer(token, pos, p, s, w) (llama2.ts:205-303): fills state.logits."""
    weights.ctx.forward(token, pos)


def argmax(arr):
    """argmax (llama2.ts:364-366): first maximum (strict '>'), NaNs never win."""
    best = 0
    bv = arr[0]
    a = np.asarray(arr)
    # numpy's argmax returns the first maximum too; NaN handling differs, so guard
    if not np.isnan(a).any():
        return int(np.argmax(a))
    for i in range(1, a.size):
        if a[i] > bv:
            best, bv = i, a[i]
    return best


def load_checkpoint_native(path, device=0):
    """Same as load_checkpoint but through l2_load_checkpoint (pinned double-buffered streaming)."""
    h = C.c_void_p()
    n = C.c_uint64()
    _check(lib().l2_load_checkpoint(path.encode(), device, 0, 1, None, C.byref(h), C.byref(n)))
    hdr = (C.c_int32 * 7)()
    _check(lib().l2_get_header(h, hdr))
    ctx = Context.__new__(Context)
    ctx.cfg = Config(tuple(hdr))
    ctx._h, ctx.tp_rank, ctx.tp_size, ctx._logits_view = h, 0, 1, None
    with open(path, "rb") as f:                     # a version-1 export is loaded with F_GQA | F_GENERATE_ROPE (include/llama2_hip.h)
        ctx.flags = (F_GQA | F_GENERATE_ROPE) if f.read(4) == b"24ka" else 0
    weights = TransformerWeights(ctx)
    return ctx.cfg, newRunState(ctx.cfg, weights), weights, n.value


def load_checkpoint(path, device=0):
    """main()'s load sequence (llama2.ts:427-436, 451) -> (config, state, weights)."""
    with open(path, "rb") as f:
        config = readConfig(f.read(28))
        weights = readWeights(config, f, device)
    return config, newRunState(config, weights), weights
