"""Spectrogram transforms on either side of the sampler.

Mirror of the transform half of the reference's ``SpecsDataModule`` (flowmse/data_module.py:149-205): STFT with
n_fft 510 (256 bins), hop 128, periodic Hann, centred frames, and the magnitude compression
``c * |z|^e * exp(j arg z)`` (e = 0.5, c = 0.15) with its inverse.  These are the "next" rows of the hot-path scope
(SURVEY.md section 8(f)); they run as torch ops (plumbing) on the device of the signal.  Dataset / dataloader code
of the reference is training infrastructure and is not reproduced.
"""
import torch


def _window(kind, n_fft):
    base = torch.hann_window(n_fft, periodic=True)
    if kind == "hann":
        return base
    if kind == "sqrthann":
        return base.sqrt()
    raise NotImplementedError(f"Window type {kind} not implemented!")


class SpecTransform:
    def __init__(self, n_fft=510, hop_length=128, window="hann", spec_factor=0.15, spec_abs_exponent=0.5,
                 transform_type="exponent", **_unused):
        if transform_type not in ("exponent", "log", "none"):
            raise ValueError(f"unknown transform_type {transform_type!r}")
        self.n_fft, self.hop_length = n_fft, hop_length
        self.window = _window(window, n_fft)
        self._win_cache = {}
        self.spec_factor, self.spec_abs_exponent = spec_factor, spec_abs_exponent
        self.transform_type = transform_type

    def _win(self, ref):
        if ref.device not in self._win_cache:
            self._win_cache[ref.device] = self.window.to(ref.device)
        return self._win_cache[ref.device]

    # ---- magnitude warping, phase preserved ---------------------------------------------------
    @staticmethod
    def _remag(spec, new_mag):
        return torch.polar(new_mag, spec.angle())

    def spec_fwd(self, spec):
        kind, c = self.transform_type, self.spec_factor
        if kind == "none":
            return spec
        if kind == "log":
            return c * self._remag(spec, torch.log1p(spec.abs()))
        e = self.spec_abs_exponent
        return c * (spec if e == 1 else self._remag(spec, spec.abs().pow(e)))

    def spec_back(self, spec):
        kind = self.transform_type
        if kind == "none":
            return spec
        spec = spec / self.spec_factor
        if kind == "log":
            return self._remag(spec, torch.expm1(spec.abs()))
        e = self.spec_abs_exponent
        return spec if e == 1 else self._remag(spec, spec.abs().pow(1.0 / e))

    # ---- fused HIP path (GPU tensors, reference STFT geometry) ------------------------------------
    def fused_ok(self, ref):
        """The HIP kernels cover the released configuration: n_fft 510, hop 128, hann, 'exponent' transform."""
        return (ref.is_cuda and self.n_fft == 510 and self.hop_length == 128 and self.transform_type == "exponent"
                and bool(torch.equal(self.window, torch.hann_window(510, periodic=True))))

    def analyze(self, sig, scale=1.0, pad_multiple=64):
        """pad_spec(spec_fwd(stft(sig * scale)))[:, None] in one kernel: sig float32 [B, L] on 'cuda' ->
        complex64 [B, 1, 256, Tpad] (frames beyond L // 128 + 1 are the zero padding)."""
        from flowmse_amd import _lib
        sig = sig.contiguous().float()
        B, L = sig.shape
        T = L // self.hop_length + 1
        Tpad = ((T + pad_multiple - 1) // pad_multiple) * pad_multiple
        out = torch.empty(B, 1, 256, Tpad, dtype=torch.complex64, device=sig.device)
        with torch.cuda.device(sig.device):
            _lib.check(_lib.lib.flowse_stft_compress(_lib.ptr(sig), B, L, float(scale), _lib.ptr(out), T, Tpad,
                                                     float(self.spec_factor), float(self.spec_abs_exponent),
                                                     _lib.current_stream()))
        return out

    def synthesize(self, spec, length, scale=1.0):
        """istft(spec_back(spec), length) * scale in one kernel: spec complex64 [B, 1, 256, Tpad] -> [B, length].
        Like the reference (model.py:190-191 on the padded sample), ALL Tpad frames take part in the overlap-add:
        the frames past length // 128 + 1 still reach the last samples of the waveform."""
        from flowmse_amd import _lib
        spec = spec.contiguous()
        B, _, F, Tpad = spec.shape
        T = Tpad
        out = torch.empty(B, length, dtype=torch.float32, device=spec.device)
        with torch.cuda.device(spec.device):
            _lib.check(_lib.lib.flowse_istft_decompress(_lib.ptr(spec), B, T, Tpad, float(self.spec_factor),
                                                        float(self.spec_abs_exponent), _lib.ptr(out), length,
                                                        float(scale), _lib.current_stream()))
        return out

    # ---- one recording as overlapping chunks (flowmse_amd.chunked) -----------------------------------
    def analyze_chunks(self, sig, Tc, hop, scale=1.0):
        """The chunk rows of ONE recording in one kernel: sig float32 [1, L] on 'cuda' -> complex64 [K, 1, 256, Tc], row k
        = frames [k hop, k hop + Tc) of ``analyze(sig)`` bit for bit (zeros past L // 128 + 1), K the chunk count of
        ``chunked.plan_chunks(L // 128 + 1, Tc, Tc - hop)``."""
        from flowmse_amd import _lib
        from flowmse_amd.chunked import plan_chunks
        sig = sig.contiguous().float()
        if sig.dim() != 2 or sig.shape[0] != 1:
            raise ValueError(f"analyze_chunks takes one recording [1, L], got {tuple(sig.shape)}")
        L = sig.shape[1]
        K, hop, _ = plan_chunks(L // self.hop_length + 1, Tc, Tc - hop)
        out = torch.empty(K, 1, 256, Tc, dtype=torch.complex64, device=sig.device)
        with torch.cuda.device(sig.device):
            _lib.check(_lib.lib.flowse_stft_compress_chunks(_lib.ptr(sig), L, float(scale), _lib.ptr(out), K, Tc, hop,
                                                            float(self.spec_factor), float(self.spec_abs_exponent),
                                                            _lib.current_stream()))
        return out

    def synthesize_chunks(self, chunks, hop, length, scale=1.0):
        """Cross-fade + spec_back + istft + rescale in one kernel: chunks complex64 [K, 1, 256, Tc] that start ``hop``
        frames apart -> [1, length].  The Tc - hop shared frames are blended linearly on the compressed values
        (``chunked.blend_chunks_reference`` states the rule); all (K - 1) hop + Tc frames take part in the overlap-add."""
        from flowmse_amd import _lib
        chunks = chunks.contiguous()
        K, _, F, Tc = chunks.shape
        out = torch.empty(1, length, dtype=torch.float32, device=chunks.device)
        with torch.cuda.device(chunks.device):
            _lib.check(_lib.lib.flowse_istft_decompress_chunks(_lib.ptr(chunks), K, Tc, int(hop), float(self.spec_factor),
                                                               float(self.spec_abs_exponent), _lib.ptr(out), length,
                                                               float(scale), _lib.current_stream()))
        return out

    # ---- one recording as trailing chunks (flowmse_amd.chunked.enhance_trailing) ----------------------
    def analyze_trailing(self, sig, Tc, H, scale=1.0):
        """The trailing rows of ONE recording in one kernel: sig float32 [1, L] on 'cuda' -> complex64 [K, 1, 256, Tc], row k
        = frames [k H - P, k H + H) of ``analyze(sig)`` bit for bit, P = Tc - H, zeros before frame 0 and past L // 128 + 1;
        K = ``chunked.plan_trailing(L // 128 + 1, Tc, H, 0)[0]``."""
        from flowmse_amd import _lib
        from flowmse_amd.chunked import plan_trailing
        sig = sig.contiguous().float()
        if sig.dim() != 2 or sig.shape[0] != 1:
            raise ValueError(f"analyze_trailing takes one recording [1, L], got {tuple(sig.shape)}")
        L = sig.shape[1]
        K = plan_trailing(L // self.hop_length + 1, Tc, H, 0)[0]
        out = torch.empty(K, 1, 256, int(Tc), dtype=torch.complex64, device=sig.device)
        with torch.cuda.device(sig.device):
            _lib.check(_lib.lib.flowse_stft_compress_trailing(_lib.ptr(sig), L, float(scale), _lib.ptr(out), K, int(Tc), int(H),
                                                              float(self.spec_factor), float(self.spec_abs_exponent),
                                                              _lib.current_stream()))
        return out

    def synthesize_trailing(self, chunks, H, X, length, scale=1.0):
        """Trailing seam rule + spec_back + istft + rescale in one kernel: chunks complex64 [K, 1, 256, Tc] that slide by
        ``H`` frames and cross-fade over ``X`` -> [1, length] (``chunked.blend_trailing_reference`` states the rule); all
        K H frames take part in the overlap-add."""
        from flowmse_amd import _lib
        chunks = chunks.contiguous()
        K, _, F, Tc = chunks.shape
        out = torch.empty(1, length, dtype=torch.float32, device=chunks.device)
        with torch.cuda.device(chunks.device):
            _lib.check(_lib.lib.flowse_istft_decompress_trailing(_lib.ptr(chunks), K, Tc, int(H), int(X),
                                                                 float(self.spec_factor), float(self.spec_abs_exponent),
                                                                 _lib.ptr(out), length, float(scale), _lib.current_stream()))
        return out

    # ---- rows and stacks from many recordings (flowmse_amd.pooled) ------------------------------------
    def analyze_rows(self, rows, Tw):
        """The input rows of ONE sampler call from several signals in one kernel: ``rows`` is a list of
        ``(sig, frame0, scale)`` with ``sig`` a 1-D float32 'cuda' tensor (two rows may share one) -> complex64
        [R, 1, 256, Tw], row r = frames [frame0, frame0 + Tw) of ``analyze(sig[None], scale)`` bit for bit (zeros past
        L // 128 + 1).  1 <= R <= 64 (``FLOWSE_MAX_SPEC_ROWS``: the table travels in the kernel's argument block)."""
        from flowmse_amd import _lib
        R = len(rows)
        if not 1 <= R <= _lib.FLOWSE_MAX_SPEC_ROWS:
            raise ValueError(f"analyze_rows takes 1..{_lib.FLOWSE_MAX_SPEC_ROWS} rows, got {R}")
        device = rows[0][0].device
        table = (_lib.flowse_spec_row * R)()
        for d, (sig, frame0, scale) in zip(table, rows):
            if sig.dim() != 1 or sig.dtype != torch.float32 or not sig.is_contiguous() or sig.device != device:
                raise ValueError(f"analyze_rows: every signal is a contiguous 1-D float32 tensor on {device}, got "
                                 f"{sig.dtype} {tuple(sig.shape)} on {sig.device}")
            d.sig, d.L, d.frame0, d.scale_in = sig.data_ptr(), sig.numel(), int(frame0), float(scale)
        out = torch.empty(R, 1, 256, int(Tw), dtype=torch.complex64, device=device)
        with torch.cuda.device(device):
            _lib.check(_lib.lib.flowse_stft_compress_rows(table, R, int(Tw), _lib.ptr(out), float(self.spec_factor),
                                                          float(self.spec_abs_exponent), _lib.current_stream()))
        return out

    def synthesize_stacks(self, chunks, S, hop, length, scale=1.0):
        """``synthesize_chunks`` for S chunk stacks of one geometry in one kernel: chunks complex64 [S * K, 1, 256, Tc],
        rows ordered (stack, chunk) -> [S, length], row s bit for bit ``synthesize_chunks`` of stack s."""
        from flowmse_amd import _lib
        chunks = chunks.contiguous()
        S = int(S)
        rows, _, F, Tc = chunks.shape
        if S < 1 or rows % S:
            raise ValueError(f"synthesize_stacks: {rows} chunk rows do not make {S} equal stacks")
        out = torch.empty(S, length, dtype=torch.float32, device=chunks.device)
        with torch.cuda.device(chunks.device):
            _lib.check(_lib.lib.flowse_istft_decompress_stacks(_lib.ptr(chunks), S, rows // S, Tc, int(hop),
                                                               float(self.spec_factor), float(self.spec_abs_exponent),
                                                               _lib.ptr(out), length, float(scale), _lib.current_stream()))
        return out

    def synthesize_ensemble(self, chunks, S, D, hop, length, scale=1.0, *, stack_stride=None, draw_stride=None, tracks=False,
                            K=None):
        """``synthesize_stacks`` over ``D`` draws per stack in one kernel (``flowmse_amd.ensemble`` has the definitions): the
        waveform of the MEAN of the draws' linear spectra, each draw blended and decompressed on its own -> [S, length]; with
        ``tracks`` also float32 [S, 2, Tg]: per frame the draws' deviation from the mean, then the mean's power.  Chunk k of
        draw d of stack s is row ``s * stack_stride + d * draw_stride + k`` of ``chunks`` [rows, 1, 256, Tc]; the default is
        the contiguous [S][D][K] layout (``stack_stride = D K``, ``draw_stride = K``).  ``K`` defaults to
        ``rows // (S D)``; name it when the rows hold more than the S D K that are read.  ``D == 1`` is ``synthesize_stacks``
        bit for bit and has no tracks."""
        from flowmse_amd import _lib
        chunks = chunks.contiguous()
        S, D = int(S), int(D)
        rows, _, F, Tc = chunks.shape
        if S < 1 or D < 1 or (K is None and rows % (S * D)):
            raise ValueError(f"synthesize_ensemble: {rows} chunk rows do not make {S} stacks of {D} draws")
        K = rows // (S * D) if K is None else int(K)
        if tracks and D < 2:
            raise ValueError("synthesize_ensemble: the tracks need D >= 2 draws")
        stack_stride = D * K if stack_stride is None else int(stack_stride)
        draw_stride = K if draw_stride is None else int(draw_stride)
        if K < 1 or min(stack_stride, draw_stride) < 0 or (S - 1) * stack_stride + (D - 1) * draw_stride + K > rows:
            raise ValueError(f"synthesize_ensemble: S={S} D={D} K={K} stack_stride={stack_stride} draw_stride={draw_stride} "
                             f"reads past the {rows} rows given")
        out = torch.empty(S, length, dtype=torch.float32, device=chunks.device)
        Tg = (K - 1) * int(hop) + Tc
        tr = torch.empty(S, 2, Tg, dtype=torch.float32, device=chunks.device) if tracks else None
        with torch.cuda.device(chunks.device):
            _lib.check(_lib.lib.flowse_istft_decompress_ensemble(_lib.ptr(chunks), S, D, K, Tc, int(hop), stack_stride,
                                                                 draw_stride, float(self.spec_factor),
                                                                 float(self.spec_abs_exponent), _lib.ptr(out), length,
                                                                 float(scale), _lib.ptr(tr), _lib.current_stream()))
        return (out, tr) if tracks else out

    # ---- STFT pair ------------------------------------------------------------------------------
    def _stft_args(self, ref):
        return dict(n_fft=self.n_fft, hop_length=self.hop_length, window=self._win(ref), center=True)

    def stft(self, sig):
        return torch.stft(sig, return_complex=True, **self._stft_args(sig))

    def istft(self, spec, length=None):
        return torch.istft(spec, length=length, **self._stft_args(spec))
