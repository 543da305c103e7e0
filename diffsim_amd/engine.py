"""Python handle over the C ABI: U-Net-to-tap engine, fused score tail and single-op entry points.

PyTorch is used only as the owner of device memory and streams; all arithmetic happens in
libdiffsim_amd.so.  Every call passes ``tensor.data_ptr()`` and the current HIP stream.
"""
from __future__ import annotations

import ctypes as C
import math
import threading
from typing import Dict, List, NamedTuple, Optional, Tuple

import torch

from . import _lib
from .config import UNetConfig

_TORCH2DSIM = {torch.float32: _lib.DSIM_F32, torch.bfloat16: _lib.DSIM_BF16, torch.float16: _lib.DSIM_F16}


def _stream_ptr() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _require_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise _lib.DsimError("tensor is not on the GPU: the engine has no CPU path")
        if t is not None and not t.is_contiguous():
            raise _lib.DsimError("tensor must be contiguous")


def resolve_tap(cfg: UNetConfig, target_block: str, target_layer):
    """(absolute block index, attention index, transformer-block index) of the hooked attn1.
    SD1.5 (diffsim/diffsim.py:122-145): down_blocks[:-1][l] / mid / up_blocks[1:][l], always attentions[-1]
    .transformer_blocks[-1].  SDXL (diffsim/diffsim_xl.py:88-107): target_layer = [block, attention, tfm_block]
    into down_blocks[1:] / up_blocks[:-1]; mid = [attention, tfm_block]."""
    if not cfg.sdxl_tap:
        l = int(target_layer)
        if target_block == "down_blocks":
            return l, -1, -1
        if target_block == "mid_blocks":
            return 0, -1, -1
        return l + 1, -1, -1
    tl = [int(v) for v in target_layer]
    if target_block == "down_blocks":
        return tl[0] + 1, tl[1], tl[2]
    if target_block == "mid_blocks":
        return 0, tl[0], tl[1]
    return tl[0], tl[1], tl[2]


def check_ctx_table(cfg: UNetConfig, ctx: torch.Tensor, ctx_index, n_images: int):
    """The prompt contexts of one qkv / qkv_taps call, checked on the host: (n_ctx, index).  ctx is (2, L, Dc) -- one [uncond,
    cond] pair for every image -- or a table (n_ctx, 2, L, Dc) with ctx_index, image i's row: a host sequence or tensor of n_images
    values in [0, n_ctx).  index is None where one context serves every image (a table of one row, or (2, L, Dc)), else an int32
    CPU tensor."""
    L, Dc = cfg.ctx_len, cfg.cross_attention_dim
    if ctx.ndim == 3:
        if tuple(ctx.shape) != (2, L, Dc):
            raise _lib.DsimError(f"ctx must be (2, {L}, {Dc}) or a table (n_ctx, 2, {L}, {Dc})")
        n_ctx = 1
    elif ctx.ndim == 4:
        if tuple(ctx.shape[1:]) != (2, L, Dc) or ctx.shape[0] < 1:
            raise _lib.DsimError(f"a context table must be (n_ctx, 2, {L}, {Dc}), got {tuple(ctx.shape)}")
        n_ctx = int(ctx.shape[0])
        if ctx_index is None:
            raise _lib.DsimError("a context table needs ctx_index: each image's row")
    else:
        raise _lib.DsimError(f"ctx must be (2, {L}, {Dc}) or a table (n_ctx, 2, {L}, {Dc})")
    if ctx_index is None:
        return 1, None
    idx = torch.as_tensor(ctx_index).reshape(-1)
    if idx.is_floating_point() or idx.is_complex() or idx.dtype == torch.bool:
        raise _lib.DsimError("ctx_index must hold integers")
    idx = idx.cpu().to(torch.int64)
    if idx.numel() != n_images:
        raise _lib.DsimError(f"ctx_index has {idx.numel()} entries for {n_images} images")
    if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= n_ctx):
        raise _lib.DsimError(f"ctx_index values must lie in [0, {n_ctx})")
    return n_ctx, (idx.to(torch.int32) if n_ctx > 1 else None)


def _cfg_struct(cfg: UNetConfig, dtype: torch.dtype, tap_block: str, tap_layer) -> _lib.UNetCfgC:
    c = _lib.UNetCfgC()
    n = len(cfg.block_out_channels)
    c.in_channels, c.n_levels = cfg.in_channels, n
    for i in range(n):
        c.block_out_channels[i] = cfg.block_out_channels[i]
        c.down_has_attn[i] = int(cfg.down_block_types[i] == "CrossAttnDownBlock2D")
        c.up_has_attn[i] = int(cfg.up_block_types[i] == "CrossAttnUpBlock2D")
        c.heads_per_level[i] = cfg.heads(i) if cfg.heads_per_level else 0
        c.depth_per_level[i] = cfg.depth(i)
    c.layers_per_block = cfg.layers_per_block
    c.num_heads = cfg.num_attention_heads
    c.cross_attention_dim = cfg.cross_attention_dim
    c.norm_num_groups = cfg.norm_num_groups
    c.norm_eps = cfg.norm_eps
    c.sample_size = cfg.sample_size
    c.ctx_len = cfg.ctx_len
    c.compute_dtype = _TORCH2DSIM[dtype]
    c.tap_block = _lib.TAP[tap_block]
    c.tap_layer, c.tap_attn, c.tap_tfm = resolve_tap(cfg, tap_block, tap_layer)
    c.addition_embed = int(cfg.addition_embed)
    c.addition_time_embed_dim = cfg.addition_time_embed_dim
    c.pooled_dim = cfg.pooled_dim
    return c


class _Handle:
    """What the executors' Python handles share: one C handle of the dsim_<prefix>_* group (create / load_weight / finalize /
    destroy / profile*), its workspace arenas, and the search for the largest batch a dry-run planner accepts.  A subclass sets
    `prefix`, self.L and self.device, then calls _create_and_load."""

    prefix = ""

    def _fn(self, name: str):
        return getattr(self.L, f"dsim_{self.prefix}_{name}")

    def _create_and_load(self, cfg_struct, state_dict: Dict[str, torch.Tensor], keep=lambda key: True):
        """Create the handle, lend it every parameter `keep` accepts (on the device, in a dtype the library reads) and pack them."""
        self._h = C.c_void_p()
        self._ws_by_stream: Dict[int, torch.Tensor] = {}      # one arena per HIP stream the handle is driven from
        self._ws = None                                        # the arena of the latest call
        with torch.cuda.device(self.device):
            _lib.check(self._fn("create")(C.byref(cfg_struct), C.byref(self._h)), f"dsim_{self.prefix}_create")
            alive = []                                         # the library borrows the tensors until finalize
            for k, v in state_dict.items():
                if not keep(k):
                    continue
                t = v.detach()
                if t.dtype not in _TORCH2DSIM:
                    t = t.float()
                t = t.to(self.device).contiguous()
                alive.append(t)
                shp = (C.c_int64 * t.ndim)(*t.shape)
                _lib.check(self._fn("load_weight")(self._h, k.encode(), t.data_ptr(), _TORCH2DSIM[t.dtype], shp, t.ndim),
                           f"{self.prefix} load_weight({k})")
            torch.cuda.synchronize(self.device)
            _lib.check(self._fn("finalize")(self._h, _stream_ptr()), f"dsim_{self.prefix}_finalize")
            del alive

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._fn("destroy")(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def profile(self, enable: bool):
        """HIP-event brackets around every launch of the following forwards (dsim_*_profile); not inside a timed region."""
        _lib.check(self._fn("profile")(self._h, int(enable)), f"{self.prefix} profile")

    def profile_records(self, detail: bool = False):
        """[(kernel family, algorithmic flops, algorithmic bytes, ms)] of the forwards run since
        profile(True); synchronises the device first.  detail=True appends the launch's shape string."""
        torch.cuda.synchronize(self.device)
        out = []
        buf = C.create_string_buffer(160)
        fl, by, ms = C.c_double(), C.c_double(), C.c_double()
        for i in range(self._fn("profile_count")(self._h)):
            _lib.check(self._fn("profile_get")(self._h, i, buf, 160, C.byref(fl), C.byref(by), C.byref(ms)),
                       f"{self.prefix} profile_get")
            fam, _, shape = buf.value.decode().partition("|")
            out.append((fam, fl.value, by.value, ms.value, shape) if detail else (fam, fl.value, by.value, ms.value))
        return out

    @staticmethod
    def _largest(fits, upper: int) -> int:
        """Largest m in [1, upper] with fits(m), 0 if none; fits is monotone (a dry-run planner: workspace bytes > 0)."""
        if not fits(1):
            return 0
        if fits(upper):
            return upper
        lo, hi = 1, upper
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if fits(mid) else (lo, mid)
        return lo

    def _arena(self, need: int) -> torch.Tensor:
        """The calling stream's workspace, grown to `need` bytes.  The entry points keep no per-call state in the handle, so
        independent batches may be in flight on several streams at once (one host thread): each stream gets its own arena."""
        sid = _stream_ptr()
        ws = self._ws_by_stream.get(sid)
        if ws is None or ws.numel() < need:
            self._ws_by_stream.pop(sid, None)
            ws = self._ws = None                            # the old arena is freed before its replacement exists
            self._arena_replaced()
            ws = self._ws_by_stream[sid] = torch.empty(need, dtype=torch.uint8, device=self.device)
        self._ws = ws
        return ws

    def _arena_replaced(self):
        """An arena is about to be freed: whatever holds its addresses goes too."""


class UNetEngine(_Handle):
    """One handle = one (config, compute dtype, tap) triple with its own packed weights.

    Replaces ``self.unet(...)`` + the attention pre-hook of the reference
    (diffsim/diffsim_pipeline.py:213-221, diffsim/diffsim.py:43-56, 122-145).
    """

    prefix = "unet"

    def __init__(self, cfg: UNetConfig, state_dict: Dict[str, torch.Tensor], dtype: torch.dtype = torch.bfloat16,
                 target_block: str = "up_blocks", target_layer: int = 0, device: str = "cuda:0"):
        if dtype not in (torch.float32, torch.bfloat16, torch.float16):
            raise ValueError("compute dtype must be float32 (parity mode), bfloat16 or float16")
        self.L = _lib.lib()
        if not torch.cuda.is_available():
            raise _lib.DsimError("no GPU visible: the DiffSim engine runs only on the HIP device")
        self.cfg, self.dtype, self.device = cfg, dtype, torch.device(device)
        self.target_block, self.target_layer = target_block, target_layer
        self._create_and_load(_cfg_struct(cfg, dtype, target_block, target_layer), state_dict)
        self.sample_size = cfg.sample_size
        self._refresh_tap_shape()
        self._graphs: Dict[tuple, tuple] = {}
        self.use_graphs = False
        self._profiling = False
        self._t = None

    def _refresh_tap_shape(self):
        n, h, d = C.c_int(), C.c_int(), C.c_int()
        _lib.check(self.L.dsim_unet_tap_shape(self._h, C.byref(n), C.byref(h), C.byref(d)), "tap_shape")
        self.tokens, self.heads, self.head_dim = n.value, h.value, d.value
        self._max_images = None

    def set_tap(self, target_block: str, target_layer):
        """Move the tap; the packed weights are shared (one copy per dtype serves every --target_block /
        --target_layer).  Raises if a parameter needed before the new tap was never loaded."""
        if (target_block, target_layer) == (self.target_block, self.target_layer):
            return
        tl, ta, tt = resolve_tap(self.cfg, target_block, target_layer)
        _lib.check(self.L.dsim_unet_set_tap(self._h, _lib.TAP[target_block], tl, ta, tt), "dsim_unet_set_tap")
        self.target_block, self.target_layer = target_block, target_layer
        self._refresh_tap_shape()           # (captured hipGraphs are keyed by tap and latent side: a sweep that alternates
                                            #  between taps keeps both graphs instead of re-capturing at every switch)

    def set_sample_size(self, side: int):
        """Latent side of the next qkv() calls (cfg.sample_size is the default, not a limit)."""
        if side != self.sample_size:
            # any side the reference accepts (--image_size a multiple of 8, argprocess.py:8): sides that are not a multiple of
            # 2**(levels-1) take the ceil-div stride-2 convs and the explicit-size upsample (diffusers' forward_upsample_size)
            if side < 2:
                raise ValueError(f"latent side {side}: --image_size must be at least 16")
            _lib.check(self.L.dsim_unet_set_sample_size(self._h, int(side)), "dsim_unet_set_sample_size")
            self.sample_size = int(side)
            self._refresh_tap_shape()

    def _graph_changed(self):
        """The executed graph is another one: the image bounds found for the old one and the hipGraphs captured from it go."""
        self._max_images = None
        self.__dict__.pop("_max_images_taps", None)
        self.__dict__.pop("_max_images_ctx", None)
        self._graphs.clear()

    def set_cfg_dedup(self, enable: bool):
        """Opt-in: compute the part of the graph both CFG halves share once (SD1.5 graphs; bit-identical scores)."""
        _lib.check(self.L.dsim_unet_set_cfg_dedup(self._h, int(bool(enable))), "dsim_unet_set_cfg_dedup")
        self._graph_changed()

    def set_fusion(self, mask: int):
        """Which multi-operator kernels replace their unfused chains (_lib.FUSE_* bits; default all).  0 = every layer
        its own launch: the A/B switch of bench.py --fusion and of the parity tests."""
        _lib.check(self.L.dsim_unet_set_fusion(self._h, int(mask)), "dsim_unet_set_fusion")
        self._graph_changed()

    def view(self, target_block: str, target_layer) -> "TapView":
        return TapView(self, target_block, target_layer)

    def set_timestep(self, t: int):
        if self._t != t:
            with torch.cuda.device(self.device):
                _lib.check(self.L.dsim_unet_set_timestep(self._h, int(t), _stream_ptr()), "set_timestep")
            self._t = t
            self._graphs.clear()

    def set_conditioning(self, t: int, text_embeds: torch.Tensor, time_ids: torch.Tensor):
        """SDXL: timestep + added conditioning (pooled text embeds (2,P) [neg,pos], time ids (2,6))."""
        te = text_embeds.to(self.device, torch.float32).contiguous()
        ti = time_ids.to(self.device, torch.float32).contiguous()
        with torch.cuda.device(self.device):
            _lib.check(self.L.dsim_unet_set_conditioning(self._h, int(t), te.data_ptr(), ti.data_ptr(), _stream_ptr()),
                       "set_conditioning")
            torch.cuda.synchronize(self.device)     # te/ti may be freed by the caller
        self._t = ("cond", t)
        self._graphs.clear()

    def profile(self, enable: bool):
        self._profiling = bool(enable)
        super().profile(enable)

    def workspace_bytes(self, n_images: int, n_ctx: int = 1) -> int:
        """Workspace of one qkv() call over n_images with n_ctx prompt contexts (n_ctx > 1: a context table, whose per-image
        contexts and K / V rows the arena holds too); 0 when the call is impossible."""
        if n_ctx == 1:
            return int(self.L.dsim_unet_workspace_bytes(self._h, n_images))
        return int(self.L.dsim_unet_ctx_workspace_bytes(self._h, n_images, int(n_ctx)))

    def max_images(self, upper: int = 4096, n_ctx: int = 1) -> int:
        """Largest n_images one qkv() call accepts (every activation < 2 GiB); bisection over the dry-run planner,
        cached (it depends on the graph only, and on whether the call carries a context table)."""
        if n_ctx == 1:
            if getattr(self, "_max_images", None) is not None:
                return self._max_images
            self._max_images = self._largest(lambda m: self.workspace_bytes(m) > 0, upper)
            return self._max_images
        cache = self.__dict__.setdefault("_max_images_ctx", {})
        key = (self.target_block, str(self.target_layer), self.sample_size)
        if key not in cache:
            cache[key] = self._largest(lambda m: self.workspace_bytes(m, 2) > 0, upper)
        return cache[key]

    def _check_inputs(self, latents, noise, ctx):
        _require_cuda(latents, noise, ctx)
        if latents.dtype != torch.float32 or noise.dtype != torch.float32 or ctx.dtype != torch.float32:
            raise _lib.DsimError("latents, noise and ctx must be float32")
        if latents.ndim != 4 or latents.shape[1] != self.cfg.in_channels or latents.shape[2] != latents.shape[3] or \
                noise.shape != latents.shape:
            raise _lib.DsimError(f"latents and noise must be (n,{self.cfg.in_channels},s,s)")
        self.set_sample_size(int(latents.shape[2]))
        if ctx.ndim != 4 and tuple(ctx.shape) != (2, self.cfg.ctx_len, self.cfg.cross_attention_dim):
            raise _lib.DsimError("ctx must be (2, ctx_len, cross_attention_dim)")

    def _ctx_args(self, ctx, ctx_index, n):
        """(ctx, n_ctx, device index) of a call: one context -> ((2, L, Dc), 1, None), the existing entry points; a table of
        several -> (table, n_ctx, int32 index uploaded on the calling stream), after the host-side checks."""
        n_ctx, idx = check_ctx_table(self.cfg, ctx, ctx_index, n)
        if n_ctx == 1:
            return (ctx[0] if ctx.ndim == 4 else ctx), 1, None
        if self.cfg.addition_embed:
            raise _lib.DsimError("SDXL handles take one prompt per call: the pooled prompt embedding enters every resnet")
        return ctx, n_ctx, idx.to(self.device)

    def _arena_replaced(self):
        self._graphs.clear()                 # captured graphs hold the old arena's addresses

    def qkv(self, latents: torch.Tensor, noise: torch.Tensor, sqrt_abar: float, sqrt_1m_abar: float,
            ctx: torch.Tensor, out: Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]] = None, ctx_index=None):
        """latents/noise (n,Cin,s,s) f32 cuda; ctx (2,L,Dc) f32 cuda -> q,k,v each
        [n][2][tokens][heads*head_dim] in the compute dtype.  Several prompts in one forward: ctx a table (n_ctx,2,L,Dc) f32 cuda
        and ctx_index image i's row of it (host values in [0, n_ctx), checked here; check_ctx_table).  Image i's rows are then
        bit for bit those of a call with ctx = table[ctx_index[i]]; a table of one row runs the one-prompt call."""
        self._check_inputs(latents, noise, ctx)
        n = latents.shape[0]
        with torch.cuda.device(self.device):
            ctx, n_ctx, idx = self._ctx_args(ctx, ctx_index, n)
            need = self.workspace_bytes(n, n_ctx)
            if need == 0:
                raise _lib.DsimError(f"{n} images do not fit one call (an activation would reach 2 GiB): at most "
                                     f"{self.max_images(n_ctx=n_ctx)} images per call for this graph")
            self._arena(need)
            shape = (n, 2, self.tokens, self.heads * self.head_dim)
            if self.use_graphs and out is None and not self._profiling:
                return self._replay(latents, noise, float(sqrt_abar), float(sqrt_1m_abar), ctx, shape, idx)
            if out is None:
                out = tuple(torch.empty((3,) + tuple(shape), dtype=self.dtype, device=self.device).unbind(0))    # one allocation: the tapped q | k | v projection is then one launch
            self._launch(latents, noise, float(sqrt_abar), float(sqrt_1m_abar), ctx, out, idx)
        return out

    # ---- tap sweeps: the q,k,v of several taps from one forward (dsim_unet_qkv_taps) -------------------------------
    def _taps_c(self, taps):
        """[(target_block, target_layer)] in the reference's addressing (set_tap's) -> a dsim_tap array"""
        arr = (_lib.TapC * max(1, len(taps)))()
        for i, tap in enumerate(taps):
            try:
                block, layer = tap
                tl, ta, tt = resolve_tap(self.cfg, block, layer)
                arr[i].block, arr[i].layer, arr[i].attn, arr[i].tfm = _lib.TAP[block], tl, ta, tt
            except (KeyError, IndexError, TypeError, ValueError):
                raise _lib.DsimError(f"unknown tap {tap!r}") from None
        return arr

    def tap_shape(self, target_block: str, target_layer) -> Tuple[int, int, int]:
        """(tokens, heads, head_dim) of a tap at the current latent side; the handle's own tap does not move."""
        n, h, d = C.c_int(), C.c_int(), C.c_int()
        arr = self._taps_c([(target_block, target_layer)])
        _lib.check(self.L.dsim_unet_tap_shape_at(self._h, arr, C.byref(n), C.byref(h), C.byref(d)),
                   f"tap {target_block} {target_layer}")
        return n.value, h.value, d.value

    def taps_workspace_bytes(self, n_images: int, taps, n_ctx: int = 1) -> int:
        """Workspace of one qkv_taps call over n_images (0: the call is impossible -- see dsim_unet_taps_workspace_bytes);
        n_ctx > 1: with a context table (dsim_unet_taps_ctx_workspace_bytes)."""
        if n_ctx == 1:
            return int(self.L.dsim_unet_taps_workspace_bytes(self._h, n_images, len(taps), self._taps_c(taps)))
        return int(self.L.dsim_unet_taps_ctx_workspace_bytes(self._h, n_images, int(n_ctx), len(taps), self._taps_c(taps)))

    def max_images_taps(self, taps, upper: int = 4096, n_ctx: int = 1) -> int:
        """Largest n_images one qkv_taps call over `taps` accepts (every activation and tap output < 2 GiB); cached per tap set,
        latent side and whether the call carries a context table."""
        key = (tuple((b, str(l)) for b, l in taps), self.sample_size) + ((("ctx",) if n_ctx > 1 else ()))
        cache = self.__dict__.setdefault("_max_images_taps", {})
        if key not in cache:
            cache[key] = self._largest(lambda m: self.taps_workspace_bytes(m, taps, min(int(n_ctx), 2)) > 0, upper)
        return cache[key]

    def qkv_taps(self, latents: torch.Tensor, noise: torch.Tensor, sqrt_abar: float, sqrt_1m_abar: float, ctx: torch.Tensor,
                 taps, ctx_index=None) -> List[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]]:
        """qkv() at every tap of `taps` ([(target_block, target_layer)], any order, no repeats) from ONE forward to the deepest
        of them: entry i is bit for bit what qkv() returns with the tap at taps[i].  The handle's own tap does not move.  Runs
        eagerly (no hipGraph), on the calling stream's workspace arena.  ctx / ctx_index: as qkv() takes them."""
        self._check_inputs(latents, noise, ctx)
        n, nt = latents.shape[0], len(taps)
        if nt < 1:
            raise _lib.DsimError("qkv_taps: no taps")
        arr = self._taps_c(taps)
        with torch.cuda.device(self.device):
            ctx, n_ctx, idx = self._ctx_args(ctx, ctx_index, n)
            need = self.taps_workspace_bytes(n, taps, n_ctx)
            shapes = [self.tap_shape(b, l) if need else (1, 1, 1) for b, l in taps]
            if need:
                ws = self._arena(need)
            else:
                # impossible call: dsim_unet_qkv_taps names the reason (an invalid, repeated or unloaded tap) before it enqueues
                # anything; a workspace refusal means the batch is too large
                ws = torch.empty(256, dtype=torch.uint8, device=self.device)
            outs = [tuple(torch.empty((3, n, 2, t, h * d), dtype=self.dtype, device=self.device).unbind(0)) for t, h, d in shapes]
            ptr = lambda j: (C.c_void_p * nt)(*[o[j].data_ptr() for o in outs])
            if n_ctx == 1:
                st = self.L.dsim_unet_qkv_taps(self._h, latents.data_ptr(), noise.data_ptr(), float(sqrt_abar), float(sqrt_1m_abar),
                                               ctx.data_ptr(), n, nt, arr, ptr(0), ptr(1), ptr(2), ws.data_ptr(),
                                               ws.numel() if need else 0, _stream_ptr())
            else:
                st = self.L.dsim_unet_qkv_taps_ctx(self._h, latents.data_ptr(), noise.data_ptr(), float(sqrt_abar),
                                                   float(sqrt_1m_abar), ctx.data_ptr(), n_ctx, idx.data_ptr(), n, nt, arr, ptr(0),
                                                   ptr(1), ptr(2), ws.data_ptr(), ws.numel() if need else 0, _stream_ptr())
            if not need and st in (0, -3):
                raise _lib.DsimError(f"{n} images do not fit one sweep call (an activation or a tap output would reach 2 GiB): at "
                                     f"most {self.max_images_taps(taps, n_ctx=n_ctx)} images per call for these taps")
            _lib.check(st, "dsim_unet_qkv_taps")
        return outs

    # ---- the tapped block's cross-attention operands (dsim_unet_qkv_text) -------------------------------------------
    def text_workspace_bytes(self, n_images: int, n_ctx: int = 1) -> int:
        """Workspace of one qkv_text() call over n_images (0: the call is impossible, as workspace_bytes)."""
        return int(self.L.dsim_unet_text_workspace_bytes(self._h, n_images, int(n_ctx)))

    def qkv_text(self, latents: torch.Tensor, noise: torch.Tensor, sqrt_abar: float, sqrt_1m_abar: float, ctx: torch.Tensor,
                 ctx_index=None):
        """qkv() whose walk runs the tapped block on to its cross-attention: returns (q, k, v, xq, xkv) -- q, k, v bit for bit
        qkv()'s; xq [n][2][tokens][heads*head_dim], the block's attn2.to_q(norm2(h + attn1(...))); xkv [n_kv][ctx_len][2*C], its
        attn2.to_k | to_v of the prompt (n_kv = 2, [uncond, cond], for one prompt; 2n, batch element e's context in row e, with a
        context table).  What text_attention() takes.  Runs eagerly (no hipGraph) on the calling stream's workspace arena; ctx /
        ctx_index as qkv() takes them."""
        self._check_inputs(latents, noise, ctx)
        n = latents.shape[0]
        with torch.cuda.device(self.device):
            ctx, n_ctx, idx = self._ctx_args(ctx, ctx_index, n)
            need = self.text_workspace_bytes(n, n_ctx)
            if need == 0:
                raise _lib.DsimError(f"{n} images do not fit one call (an activation would reach 2 GiB): at most "
                                     f"{self.max_images(n_ctx=n_ctx)} images per call for this graph")
            ws = self._arena(need)
            C_ = self.heads * self.head_dim
            q, k, v = torch.empty((3, n, 2, self.tokens, C_), dtype=self.dtype, device=self.device).unbind(0)   # one allocation, as qkv()
            xq = torch.empty((n, 2, self.tokens, C_), dtype=self.dtype, device=self.device)
            xkv = torch.empty((2 if n_ctx == 1 else 2 * n, self.cfg.ctx_len, 2 * C_), dtype=self.dtype, device=self.device)
            _lib.check(self.L.dsim_unet_qkv_text(self._h, latents.data_ptr(), noise.data_ptr(), float(sqrt_abar), float(sqrt_1m_abar),
                                                 ctx.data_ptr(), n_ctx, _ptr(idx), n, q.data_ptr(), k.data_ptr(), v.data_ptr(),
                                                 xq.data_ptr(), xkv.data_ptr(), ws.data_ptr(), ws.numel(), _stream_ptr()),
                       "dsim_unet_qkv_text")
        return q, k, v, xq, xkv

    def _launch(self, latents, noise, sa, sb, ctx, out, idx=None):
        q, k, v = out
        if idx is None:
            _lib.check(self.L.dsim_unet_qkv(self._h, latents.data_ptr(), noise.data_ptr(), sa, sb, ctx.data_ptr(),
                                            latents.shape[0], q.data_ptr(), k.data_ptr(), v.data_ptr(), self._ws.data_ptr(),
                                            self._ws.numel(), _stream_ptr()), "dsim_unet_qkv")
            return
        _lib.check(self.L.dsim_unet_qkv_ctx(self._h, latents.data_ptr(), noise.data_ptr(), sa, sb, ctx.data_ptr(), ctx.shape[0],
                                            idx.data_ptr(), latents.shape[0], q.data_ptr(), k.data_ptr(), v.data_ptr(),
                                            self._ws.data_ptr(), self._ws.numel(), _stream_ptr()), "dsim_unet_qkv_ctx")

    def _replay(self, latents, noise, sa, sb, ctx, shape, idx=None):
        """hipGraph path for launch-bound small batches: the ~330 kernel launches of one forward are captured
        once per (n_images, sqrt_abar, sqrt_1m_abar, n_ctx) over static input/output buffers and replayed as one graph
        launch.  dsim_unet_qkv never allocates or synchronises, so plain stream capture works.  The context table and the
        per-image index are static buffers too, refreshed before every replay like the latents: a replay never reuses the
        prompt assignment of its capture."""
        n_ctx = 1 if idx is None else int(ctx.shape[0])
        key = (self.target_block, str(self.target_layer), self.sample_size, _stream_ptr(), shape[0], sa, sb, n_ctx)
        ent = self._graphs.get(key)
        if ent is None:
            st = {"lat": torch.empty_like(latents), "nz": torch.empty_like(noise), "ctx": torch.empty_like(ctx),
                  "idx": None if idx is None else torch.empty_like(idx),
                  "out": tuple(torch.empty((3,) + tuple(shape), dtype=self.dtype, device=self.device).unbind(0))}
            st["lat"].copy_(latents), st["nz"].copy_(noise), st["ctx"].copy_(ctx)
            if idx is not None:
                st["idx"].copy_(idx)
            self._launch(st["lat"], st["nz"], sa, sb, st["ctx"], st["out"], st["idx"])      # eager warm-up (code objects loaded)
            torch.cuda.synchronize(self.device)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self._launch(st["lat"], st["nz"], sa, sb, st["ctx"], st["out"], st["idx"])
            ent = self._graphs[key] = (g, st)
        g, st = ent
        st["lat"].copy_(latents), st["nz"].copy_(noise), st["ctx"].copy_(ctx)
        if idx is not None:
            st["idx"].copy_(idx)
        g.replay()
        return tuple(t.clone() for t in st["out"])


class TapView:
    """One (target_block, target_layer) of a shared UNetEngine: every attribute access first moves the engine's tap
    there, so several taps can be used alternately over ONE packed weight copy."""

    def __init__(self, base: UNetEngine, target_block: str, target_layer):
        object.__setattr__(self, "_base", base)
        object.__setattr__(self, "_tap", (target_block, target_layer))

    def __getattr__(self, name):
        base = object.__getattribute__(self, "_base")
        base.set_tap(*object.__getattribute__(self, "_tap"))
        return getattr(base, name)

    def __setattr__(self, name, value):
        setattr(object.__getattribute__(self, "_base"), name, value)


_PAIR_MSGS = ("q,k,v must share dtype float32, bfloat16 or float16", "q,k,v must be [n_feat][B][N][H*D] of one shape",
              "features and indices must be contiguous")


def _check_features(ts, heads: int, shapes_ok: bool, msgs, idx=()):
    """The checks every score tail makes of its feature tensors ts = (q, ...), each [n][B][N][H*D], and pair index tensors idx: one
    dtype of the three, the caller's shape condition, contiguity, H*D against heads; msgs: the texts of the first three.  (B, N, D)."""
    q = ts[0]
    if q.dtype not in _TORCH2DSIM or any(t.dtype != q.dtype for t in ts):
        raise _lib.DsimError(msgs[0])
    if any(i.dtype != torch.int32 for i in idx):
        raise _lib.DsimError("pair indices must be int32")
    if q.ndim != 4 or not shapes_ok:
        raise _lib.DsimError(msgs[1])
    if not all(t.is_contiguous() for t in (*ts, *idx)):
        raise _lib.DsimError(msgs[2])
    _, B, N, HD = q.shape
    D = HD // heads
    if D * heads != HD:
        raise _lib.DsimError(f"H*D = {HD} is not a multiple of heads = {heads}")
    if idx and idx[0].numel() != idx[1].numel():
        raise _lib.DsimError("idx_a and idx_b must have the same length")
    return B, N, D


_SETS_MSGS = ("q,k,v of both sets must share dtype float32, bfloat16 or float16",
              "features must be [n][B][N][H*D], one geometry for both sets", "features must be contiguous")


def _check_two_sets(fa, fb, heads: int):
    """_check_features for the two sets of (q, k, v) a matrix call takes, one geometry for both: ((qa, ka, va, qb, kb, vb), B, N, D)."""
    (qa, ka, va), (qb, kb, vb) = fa, fb
    ok = ka.shape == qa.shape == va.shape and kb.shape == qb.shape == vb.shape and qa.shape[1:] == qb.shape[1:]
    ts = (qa, ka, va, qb, kb, vb)
    return (ts, *_check_features(ts, heads, ok, _SETS_MSGS))


class _TokenRows(NamedTuple):
    """How the region tails read one byte per token and image: the two forms of every dsim_*_regions / dsim_*_weights entry pair."""
    suffix: str                 # of the C entries and their workspace queries
    noun: str                   # of the refusals: "no <noun> scores for ..."
    matrix: str                 # ... and of the matrix form's
    what: str                   # the rows in the messages of their own checks
    arg: str                    # ... and the matrix forms' argument names, <arg>_a and <arg>_b
    dtypes: tuple
    dtype_rule: str


_MASKS = _TokenRows("regions", "region", "region score matrix", "the region mask", "mask", (torch.bool, torch.uint8), "bool or uint8")
_WEIGHTS = _TokenRows("weights", "soft region", "soft score matrix", "the token weights", "weights", (torch.uint8,), "uint8")


def _token_rows(form: _TokenRows, rows: torch.Tensor, n: int, N: int, what: Optional[str] = None, extent: str = "n_feat"):
    """The token rows of a region tail checked -- the form's dtypes, (n, N), contiguous: a strided row would be read as if dense --
    and as the uint8 the library reads; `what` names them and `extent` their first extent in the messages."""
    what = what or form.what
    if rows.dtype not in form.dtypes:
        raise _lib.DsimError(f"{what} must be {form.dtype_rule}")
    want = (*n, N) if isinstance(n, tuple) else (n, N)          # (a tuple: the cell forms' (n_a, n_b))
    if tuple(rows.shape) != want:
        raise _lib.DsimError(f"{what} must be ({extent}, N) = ({', '.join(map(str, want))}): {tuple(rows.shape)}")
    if not rows.is_contiguous():
        raise _lib.DsimError(f"{what} must be contiguous")
    return rows.view(torch.uint8)


def _with_extras(out, *extras):
    """out alone, or the tuple of out and the optional outputs the caller asked for (the others are None)"""
    asked = tuple(e for e in extras if e is not None)
    return (out,) + asked if asked else out


def _similarity_code(similarity: str) -> int:
    if similarity not in ("cosine", "mse"):
        raise ValueError(similarity)
    return 0 if similarity == "cosine" else 1


def _i32(shape, dev, want: bool = True):
    """an int32 output (a status, the counts) on dev, or None where the caller did not ask for it"""
    return torch.empty(shape, dtype=torch.int32, device=dev) if want else None


def _tail_call(dev, name: str, ws_shape, refusal: str, *args, query: Optional[str] = None):
    """dsim_<name>(*args, workspace, bytes, stream) on dev, on a fresh workspace of dsim_<query or name>_workspace_bytes(*ws_shape)
    bytes; 0 bytes: the library does not serve the shape, and `refusal` says which."""
    L = _lib.lib()
    with torch.cuda.device(dev):
        wsb = int(getattr(L, f"dsim_{query or name}_workspace_bytes")(*ws_shape))
        if wsb == 0:
            raise _lib.DsimError(refusal)
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        _lib.check(getattr(L, f"dsim_{name}")(*args, ws.data_ptr(), wsb, _stream_ptr()), f"dsim_{name}")


def pair_score(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, idx_a: torch.Tensor, idx_b: torch.Tensor,
               heads: int, similarity: str = "cosine", return_status: bool = False):
    """Fused score tail (diffsim/diffsim.py:177-197).  q,k,v: contiguous [n_feat][B][N][H*D] of one shape; idx: contiguous int32
    cuda [n_pairs] each, entries in [0, n_feat) (not checked: that would need a device sync).
    return_status: also return an int32 [n_pairs] tensor, 1 where the score is NaN / infinite (NaN guard)."""
    _require_cuda(q, k, v, idx_a, idx_b)
    sim = _similarity_code(similarity)
    B, N, D = _check_features((q, k, v), heads, k.shape == q.shape == v.shape, _PAIR_MSGS, (idx_a, idx_b))
    n_pairs = idx_a.numel()
    out = torch.empty(n_pairs, dtype=torch.float32, device=q.device)
    status = _i32(n_pairs, q.device, return_status)
    _tail_call(q.device, "pair_score_status" if return_status else "pair_score", (n_pairs, B, heads, N, D), "", q.data_ptr(),
               k.data_ptr(), v.data_ptr(), idx_a.data_ptr(), idx_b.data_ptr(), n_pairs, B, heads, N, D, _TORCH2DSIM[q.dtype], sim,
               out.data_ptr(), *((status.data_ptr(),) if return_status else ()), query="pair_score")
    return (out, status) if return_status else out


def pair_score_proj(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, idx_a: torch.Tensor, idx_b: torch.Tensor, heads: int,
                    similarity: str = "cosine", return_status: bool = False, *, w_out: torch.Tensor, bias: torch.Tensor):
    """The projected score tail (metrics/clip_i.py:143-159, dsim_pair_score_proj): pair_score with the hooked layer's out_proj
    applied to every attention output before the cosine / mse.  q, k, v, idx, heads, similarity, return_status: as pair_score.
    w_out: contiguous [C][C] in the features' dtype, C = H*D, rows = output features; bias: contiguous f32 [C]."""
    _require_cuda(q, k, v, idx_a, idx_b, w_out, bias)
    sim = _similarity_code(similarity)
    B, N, D = _check_features((q, k, v), heads, k.shape == q.shape == v.shape, _PAIR_MSGS, (idx_a, idx_b))
    Cc = heads * D
    if w_out.dtype != q.dtype or tuple(w_out.shape) != (Cc, Cc) or bias.dtype != torch.float32 or tuple(bias.shape) != (Cc,):
        raise _lib.DsimError(f"w_out must be {q.dtype} ({Cc}, {Cc}) and bias float32 ({Cc},)")
    n_pairs = idx_a.numel()
    out = torch.empty(n_pairs, dtype=torch.float32, device=q.device)
    status = _i32(n_pairs, q.device, return_status)
    dt = _TORCH2DSIM[q.dtype]
    _tail_call(q.device, "pair_score_proj", (n_pairs, B, heads, N, D, dt),
               f"the projected score tail does not serve n_pairs {n_pairs}, B {B}, H {heads}, N {N}, D {D}", q.data_ptr(), k.data_ptr(),
               v.data_ptr(), idx_a.data_ptr(), idx_b.data_ptr(), n_pairs, B, heads, N, D, dt, sim, w_out.data_ptr(), bias.data_ptr(),
               out.data_ptr(), _ptr(status))
    return (out, status) if return_status else out


def _pair_checks(ts, idx_a, idx_b, heads: int, region=None, similarity: Optional[str] = None):
    """What every per-token pair tail checks of its features ts = (q, k[, v]), its pair indices and its optional region, a
    (_TokenRows, rows) pair: ((B, heads, N, D), the similarity's code, the region with its rows as uint8)."""
    form, rows = region or (None, None)
    if form is not None and not rows.is_contiguous():          # (ahead of the device requirement: it needs no device)
        raise _lib.DsimError(f"{form.what} must be contiguous")
    _require_cuda(*ts, rows, idx_a, idx_b)
    sim = None if similarity is None else _similarity_code(similarity)
    B, N, D = _check_features(ts, heads, all(t.shape == ts[0].shape for t in ts), _PAIR_MSGS, (idx_a, idx_b))
    return (B, heads, N, D), sim, (region and (form, _token_rows(form, rows, ts[0].shape[0], N)))


def _pair_call(name: str, refusal: str, ts, region, idx_a, idx_b, dims, *rest, extra=None):
    """dsim_<name> over the pairs (idx_a, idx_b) of the features ts, or with a region dsim_<name>_<regions | weights>: the rows and
    n_feat go behind the features and `extra` (the counts / sums, or None) behind `rest`.  refusal: "no ... maps" for the shape."""
    B, H, N, D = dims
    n, n_feat = idx_a.numel(), ts[0].shape[0]
    shape = f"n_pairs={n} B={B} H={H} N={N} D={D}"
    args = (idx_a.data_ptr(), idx_b.data_ptr(), n, *dims, _TORCH2DSIM[ts[0].dtype], *rest)
    if region is None:
        return _tail_call(ts[0].device, name, (n, *dims), f"{refusal} for {shape}", *(t.data_ptr() for t in ts), *args)
    form, rows = region
    _tail_call(ts[0].device, f"{name}_{form.suffix}", (n_feat, n, *dims), f"{refusal} for n_feat={n_feat} {shape}",
               *(t.data_ptr() for t in ts), rows.data_ptr(), n_feat, *args, _ptr(extra))


def _pair_scores(q, k, v, idx_a, idx_b, heads, similarity, return_status, region, return_extra):
    """pair_score_regions and pair_score_weights: one score per pair over the region's rows"""
    dims, sim, region = _pair_checks((q, k, v), idx_a, idx_b, heads, region, similarity)
    n_pairs = idx_a.numel()
    out = torch.empty(n_pairs, dtype=torch.float32, device=q.device)
    status = _i32(n_pairs, q.device, return_status)
    extra = _i32(q.shape[0], q.device, return_extra)
    _pair_call("pair_score", f"no {region[0].noun} scores", (q, k, v), region, idx_a, idx_b, dims, sim, out.data_ptr(), _ptr(status),
               extra=extra)
    return _with_extras(out, status, extra)


def _pair_maps(q, k, v, idx_a, idx_b, heads, similarity, return_status, region=None, return_extra=False):
    """pair_score_maps and its two region forms: the score and its per-token terms on the full token grid"""
    dims, sim, region = _pair_checks((q, k, v), idx_a, idx_b, heads, region, similarity)
    n_pairs, N, dev = idx_a.numel(), dims[2], q.device
    score = torch.empty(n_pairs, dtype=torch.float32, device=dev)
    local = torch.empty((n_pairs, 2, N), dtype=torch.float32, device=dev)
    contrib = torch.empty((n_pairs, 2, N), dtype=torch.float32, device=dev)
    status = _i32(n_pairs, dev, return_status)
    extra = _i32(q.shape[0], dev, return_extra)
    _pair_call("pair_score_maps", f"no {region[0].noun} maps" if region else "no similarity maps", (q, k, v), region, idx_a, idx_b,
               dims, sim, score.data_ptr(), local.data_ptr(), contrib.data_ptr(), _ptr(status), extra=extra)
    return (score, local, contrib) + tuple(e for e in (status, extra) if e is not None)


def pair_score_maps(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, idx_a: torch.Tensor, idx_b: torch.Tensor,
                    heads: int, similarity: str = "cosine", return_status: bool = False):
    """The score tail kept per query token (dsim_pair_score_maps).  q,k,v: [n_feat][B][N][H*D]; idx: int32 cuda [n_pairs].
    Returns f32 device tensors (score (n,), local (n, 2, N), contrib (n, 2, N)): direction 0 on image idx_a[p]'s tokens,
    direction 1 on idx_b[p]'s; local is a token's own cosine (or mean squared difference), contrib its term of the score:
    score = 0.5 * contrib.sum((1, 2)).  return_status: also an int32 (n,) tensor, 1 where the score is NaN / infinite."""
    return _pair_maps(q, k, v, idx_a, idx_b, heads, similarity, return_status)


def pair_score_regions(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, mask: torch.Tensor, idx_a: torch.Tensor,
                       idx_b: torch.Tensor, heads: int, similarity: str = "cosine", return_status: bool = False,
                       return_counts: bool = False):
    """The score tail restricted to a token region per feature image (dsim_pair_score_regions).  q,k,v: [n_feat][B][N][H*D];
    mask: bool or uint8 cuda (n_feat, N), non-zero = the token is in its image's region; idx: int32 cuda [n_pairs].  Pair p's
    score is pair_score's on the rows of the two regions alone (ascending token order): the off tokens are neither queries nor
    keys.  Returns the f32 (n,) scores; return_status: also an int32 (n,) tensor, 1 where the score is NaN / infinite, 2 where
    a region of the pair is empty (score NaN); return_counts: also the int32 (n_feat,) region sizes."""
    return _pair_scores(q, k, v, idx_a, idx_b, heads, similarity, return_status, (_MASKS, mask), return_counts)


def pair_score_weights(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, weights_u8: torch.Tensor, idx_a: torch.Tensor,
                       idx_b: torch.Tensor, heads: int, similarity: str = "cosine", return_status: bool = False,
                       return_sums: bool = False):
    """The soft region score (dsim_pair_score_weights): pair_score_regions with a weight per token instead of a bit.  q,k,v:
    [n_feat][B][N][H*D]; weights_u8: uint8 cuda (n_feat, N), token t of image i weighs byte / 255; idx: int32 cuda [n_pairs].  A
    token of byte 0 is dropped as an off token is; a key of weight w enters both softmaxes with the logit bias ln w, and a query row
    of weight w counts w times in the cosine / mse sums.  With every byte 0 or 255 it is pair_score_regions on `weights_u8 != 0`, bit
    for bit.  Returns the f32 (n,) scores; return_status: also an int32 (n,) tensor, 1 where the score is NaN / infinite, 2 where
    an image of the pair has no weight at all (score NaN); return_sums: also the int32 (n_feat,) byte sums."""
    return _pair_scores(q, k, v, idx_a, idx_b, heads, similarity, return_status, (_WEIGHTS, weights_u8), return_sums)


def pair_score_maps_regions(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, mask: torch.Tensor, idx_a: torch.Tensor,
                            idx_b: torch.Tensor, heads: int, similarity: str = "cosine", return_status: bool = False,
                            return_counts: bool = False):
    """The region score kept per query token (dsim_pair_score_maps_regions): pair_score_maps for pair_score_regions.  q,k,v, mask,
    idx: as pair_score_regions.  Returns f32 device tensors (score (n,), local (n, 2, N), contrib (n, 2, N)) on the full token
    grid: at an on token, local is the token's own cosine (or mean squared difference) inside the region attention and contrib
    its term of the region score, score = 0.5 * contrib.sum((1, 2)); at an off token both are exactly 0.  return_status: also an
    int32 (n,) tensor, 1 where the score is NaN / infinite, 2 where a region of the pair is empty (score NaN, maps zero);
    return_counts: also the int32 (n_feat,) region sizes."""
    return _pair_maps(q, k, v, idx_a, idx_b, heads, similarity, return_status, (_MASKS, mask), return_counts)


def pair_score_maps_weights(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, weights_u8: torch.Tensor, idx_a: torch.Tensor,
                            idx_b: torch.Tensor, heads: int, similarity: str = "cosine", return_status: bool = False,
                            return_sums: bool = False):
    """The soft region score kept per query token (dsim_pair_score_maps_weights): pair_score_maps_regions for pair_score_weights.
    q,k,v, weights_u8, idx: as pair_score_weights.  Returns f32 device tensors (score (n,), local (n, 2, N), contrib (n, 2, N)) on the
    full token grid: at a token of weight > 0, local is the token's own cosine (or mean squared difference) inside the biased
    attentions, not weighted by its own weight, and contrib its weighted term of the soft score, score = 0.5 * contrib.sum((1, 2));
    at a token of weight 0 both are exactly 0.  With every byte 0 or 255 the outputs are pair_score_maps_regions' bits.
    return_status: also an int32 (n,) tensor, 1 where the score is NaN / infinite, 2 where an image of the pair has no weight
    (score NaN, maps zero); return_sums: also the int32 (n_feat,) byte sums."""
    return _pair_maps(q, k, v, idx_a, idx_b, heads, similarity, return_status, (_WEIGHTS, weights_u8), return_sums)


TEXT_WANT = ("attn", "saliency", "mask", "counts", "status")


def text_attention(xq: torch.Tensor, xkv: torch.Tensor, heads: int, token_weight: Optional[torch.Tensor] = None,
                   rel_threshold: float = 1.0, want=("saliency", "mask", "counts")):
    """Text attention maps and text-guided regions (dsim_text_attention) from UNetEngine.qkv_text's operands.  xq
    [n][2][N][H*D], xkv [n_kv][L][2*H*D] (K in the first H*D columns), n_kv = 2 or 2n.  On the conditional CFG half of image i,
    T_i[n][l] = the softmax over the L prompt tokens averaged over the heads, saliency s_i = T_i @ w_i with token_weight w f32
    (L,) shared or (n, L) per image, and the region: the tokens with s_i[n] >= rel_threshold * mean(s_i), or every token when none
    passes.  Returns a dict of the outputs named in `want`: attn f32 (n, N, L), saliency f32 (n, N), mask bool (n, N), counts
    int32 (n,), status int32 (n,) (1: a non-finite probability).  The values do not depend on `want`."""
    want = tuple(want)
    if not want or any(w not in TEXT_WANT for w in want):
        raise ValueError(f"want must name some of {TEXT_WANT}: {want}")
    _require_cuda(xq, xkv)
    if xq.dtype not in _TORCH2DSIM or xkv.dtype != xq.dtype:
        raise _lib.DsimError("xq and xkv must share dtype float32, bfloat16 or float16")
    if xq.ndim != 4 or xq.shape[1] != 2 or xkv.ndim != 3 or xkv.shape[2] != 2 * xq.shape[3] or xq.shape[3] % heads:
        raise _lib.DsimError(f"xq must be [n][2][N][H*D] and xkv [n_kv][L][2*H*D]: {tuple(xq.shape)}, {tuple(xkv.shape)}")
    if not (xq.is_contiguous() and xkv.is_contiguous()):
        raise _lib.DsimError("xq and xkv must be contiguous")
    n, _, N, HD = xq.shape
    n_kv, L = int(xkv.shape[0]), int(xkv.shape[1])
    dev = xq.device
    needs_w = any(w in want for w in ("saliency", "mask", "counts"))
    n_w = 1
    if token_weight is not None:
        token_weight = token_weight.to(device=dev, dtype=torch.float32).contiguous()
        if token_weight.ndim == 1:
            token_weight = token_weight[None]
        if token_weight.ndim != 2 or token_weight.shape[1] != L or token_weight.shape[0] not in (1, n):
            raise _lib.DsimError(f"token_weight must be ({L},) or ({n}, {L}): {tuple(token_weight.shape)}")
        n_w = int(token_weight.shape[0])
    elif needs_w:
        raise _lib.DsimError("saliency and regions need token_weight")
    out = {}
    if "attn" in want:
        out["attn"] = torch.empty((n, N, L), dtype=torch.float32, device=dev)
    if "saliency" in want:
        out["saliency"] = torch.empty((n, N), dtype=torch.float32, device=dev)
    if "mask" in want:
        out["mask"] = torch.empty((n, N), dtype=torch.uint8, device=dev)
    for name in ("counts", "status"):
        if name in want:
            out[name] = _i32(n, dev)
    _tail_call(dev, "text_attention", (n, N, L), f"no text attention for n={n} N={N} L={L} (1 <= L <= 128)", xq.data_ptr(), HD,
               xkv.data_ptr(), 2 * HD, n, n_kv, heads, N, L, HD // heads, _TORCH2DSIM[xq.dtype], _ptr(token_weight), n_w,
               float(rel_threshold), _ptr(out.get("attn")), _ptr(out.get("saliency")), _ptr(out.get("mask")), _ptr(out.get("counts")),
               _ptr(out.get("status")))
    if "mask" in out:
        out["mask"] = out["mask"].view(torch.bool)
    return out


_ATTN_BYTES = (1 << 31) - 1          # dsim_pair_align refuses an attention tensor of 2 GiB or more: the pairs are chunked
_ALIGN_PAIRS = 32767                 # ... and more pairs than its grid holds (two directions per pair, 65535 in all)


def _align_chunks(n_pairs: int, N: int, with_attention: bool = False):
    """The slices of n_pairs pairs that one alignment or transfer launch takes: at most _ALIGN_PAIRS, and with the (2, N, N) f32
    attention of every pair written out, fewer than 2 GiB of it."""
    step = _ALIGN_PAIRS
    if with_attention:
        step = min(step, _ATTN_BYTES // (2 * N * N * 4))
        if step < 1:
            raise _lib.DsimError(f"the attention of one pair of {N} tokens does not fit 2 GiB")
    return [slice(i0, min(n_pairs, i0 + step)) for i0 in range(0, n_pairs, step)]


def _at(t: Optional[torch.Tensor], sl: slice) -> Optional[int]:
    return None if t is None else t[sl].data_ptr()


def _pair_align(q, k, idx_a, idx_b, heads, grid_w, return_attention, return_status, region=None, return_extra=False):
    """pair_align and its two region forms"""
    dims, _, region = _pair_checks((q, k), idx_a, idx_b, heads, region)
    N = dims[2]
    if grid_w is None:
        grid_w = math.isqrt(N)
        if grid_w * grid_w != N:
            raise _lib.DsimError(f"{N} tokens do not form a square grid: name grid_w")
    n_pairs, dev = idx_a.numel(), q.device
    match = torch.empty((n_pairs, 2, N), dtype=torch.int32, device=dev)
    weight = torch.empty((n_pairs, 2, N), dtype=torch.float32, device=dev)
    expect = torch.empty((n_pairs, 2, N, 2), dtype=torch.float32, device=dev)
    status = _i32(n_pairs, dev, return_status)
    extra = _i32(q.shape[0], dev, return_extra)
    chunks = _align_chunks(n_pairs, N, return_attention)
    attn = torch.empty((n_pairs, 2, N, N), dtype=torch.float32, device=dev) if return_attention else None
    for sl in chunks:
        _pair_call("pair_align", f"no {region[0].noun} alignments" if region else "no token alignments", (q, k), region, idx_a[sl],
                   idx_b[sl], dims, int(grid_w), match[sl].data_ptr(), weight[sl].data_ptr(), expect[sl].data_ptr(), _at(attn, sl),
                   _at(status, sl), extra=extra)
    return (match, weight, expect) + tuple(e for e in (attn, status, extra) if e is not None)


def pair_align(q: torch.Tensor, k: torch.Tensor, idx_a: torch.Tensor, idx_b: torch.Tensor, heads: int,
               grid_w: Optional[int] = None, return_attention: bool = False, return_status: bool = False):
    """Token alignments (dsim_pair_align): the cross-attention the score is built on, softmax(Q_a K_b^T / sqrt(D)) averaged over
    the CFG halves and the heads.  q,k: [n_feat][B][N][H*D]; idx: int32 cuda [n_pairs].  Returns device tensors (match int32
    (n, 2, N), weight f32 (n, 2, N), expect f32 (n, 2, N, 2)): for query token i of direction 0 (image idx_a[p]'s tokens over
    idx_b[p]'s; direction 1 the mirror) the other image's token with the largest mean probability (ties: the lowest), that
    probability, and the soft-argmax (row, col) on the other image's grid, token j at (j // grid_w, j % grid_w).  grid_w None:
    the square grid of N tokens.  return_attention: also the probabilities, f32 (n, 2, N, N), computed in calls of fewer than
    2 GiB each; return_status: also an int32 (n,) tensor, 1 where a pair has a non-finite probability."""
    return _pair_align(q, k, idx_a, idx_b, heads, grid_w, return_attention, return_status)


def pair_align_regions(q: torch.Tensor, k: torch.Tensor, mask: torch.Tensor, idx_a: torch.Tensor, idx_b: torch.Tensor, heads: int,
                       grid_w: Optional[int] = None, return_attention: bool = False, return_status: bool = False,
                       return_counts: bool = False):
    """Token alignments between two regions (dsim_pair_align_regions): pair_align with the softmax of query token i in R_a taken
    over the keys j in R_b only.  q,k, idx, grid_w: as pair_align; mask: as pair_score_regions.  Returns device tensors (match
    int32 (n, 2, N), weight f32 (n, 2, N), expect f32 (n, 2, N, 2)) on the full token grid: match and expect are token indices
    and (row, col) coordinates of the other image's full grid.  Off query tokens carry match -1, weight 0, expect (-1, -1).
    return_attention: also the probabilities, f32 (n, 2, N, N), zero outside R_a x R_b, computed in calls of fewer than 2 GiB
    each; return_status: also an int32 (n,) tensor, 1 where a pair has a non-finite probability, 2 where a region of the pair is
    empty (every row then carries the off values); return_counts: also the int32 (n_feat,) region sizes."""
    return _pair_align(q, k, idx_a, idx_b, heads, grid_w, return_attention, return_status, (_MASKS, mask), return_counts)


def pair_align_weights(q: torch.Tensor, k: torch.Tensor, weights_u8: torch.Tensor, idx_a: torch.Tensor, idx_b: torch.Tensor, heads: int,
                       grid_w: Optional[int] = None, return_attention: bool = False, return_status: bool = False,
                       return_sums: bool = False):
    """Soft region alignments (dsim_pair_align_weights): pair_align_regions with the softmax of a query token taken over the keys of
    weight > 0 with ln(weight) added to each logit.  q,k, idx, grid_w: as pair_align; weights_u8: as pair_score_weights.  A query
    token's own weight does not enter; query tokens of weight 0 carry match -1, weight 0, expect (-1, -1).  Returns (match int32
    (n, 2, N), weight f32 (n, 2, N), expect f32 (n, 2, N, 2)) on the full token grid.  return_attention: also the probabilities, f32
    (n, 2, N, N), zero at rows and columns of weight 0, in calls of fewer than 2 GiB each; return_status: also an int32 (n,) tensor, 1
    where a pair has a non-finite probability, 2 where an image of the pair has no weight; return_sums: also the int32 (n_feat,) byte
    sums.  With every byte 0 or 255 the outputs are pair_align_regions' bits."""
    return _pair_align(q, k, idx_a, idx_b, heads, grid_w, return_attention, return_status, (_WEIGHTS, weights_u8), return_sums)


def pair_region_transfer(q: torch.Tensor, k: torch.Tensor, weights_u8: torch.Tensor, idx_a: torch.Tensor, idx_b: torch.Tensor, heads: int,
                         directions: int = 3, return_status: bool = False):
    """Region transfer (dsim_pair_region_transfer): the attention mass each token sends into the other image's weighted tokens,
    sum_j Pm[i][j] w[j] with pair_align's Pm (the softmax over all keys) and w = byte / 255, without forming Pm.  q,k, idx: as
    pair_align; weights_u8: as pair_score_weights.  Returns f32 (n, 2, N): row [p][0] on image idx_a[p]'s grid (its queries over
    idx_b[p]'s keys and weights), row [p][1] the mirror.  directions 1: rows [p][0] only, 2: rows [p][1] only, 3: both; the rows not
    asked for hold NaN.  return_status: also an int32 (n,) tensor, 1 where a pair has a non-finite probability."""
    _require_cuda(q, k, weights_u8, idx_a, idx_b)
    B, N, D = _check_features((q, k), heads, k.shape == q.shape, _PAIR_MSGS, (idx_a, idx_b))
    _token_rows(_WEIGHTS, weights_u8, q.shape[0], N)
    if directions not in (1, 2, 3):
        raise ValueError(f"directions must be 1, 2 or 3: {directions!r}")
    n_feat, n_pairs = q.shape[0], idx_a.numel()
    dev = q.device
    mass = torch.full((n_pairs, 2, N), float("nan"), dtype=torch.float32, device=dev)
    status = _i32(n_pairs, dev, return_status)
    for sl in _align_chunks(n_pairs, N):
        n = sl.stop - sl.start
        _tail_call(dev, "pair_region_transfer", (n_feat, n, B, heads, N, D),
                   f"no region transfer for n_feat={n_feat} n_pairs={n} B={B} H={heads} N={N} D={D}", q.data_ptr(), k.data_ptr(),
                   weights_u8.data_ptr(), n_feat, idx_a[sl].data_ptr(), idx_b[sl].data_ptr(), n, B, heads, N, D, _TORCH2DSIM[q.dtype],
                   int(directions), mass[sl].data_ptr(), _at(status, sl))
    return (mass, status) if return_status else mass


def region_transfer_matrix_workspace_bytes(n_a: int, n_b: int, B: int, heads: int, N: int, D: int, dtype: torch.dtype) -> int:
    return int(_lib.lib().dsim_region_transfer_matrix_workspace_bytes(n_a, n_b, B, heads, N, D, _TORCH2DSIM.get(dtype, -1)))


def region_transfer_matrix(fa, fb, weights_a: torch.Tensor, heads: int, return_status: bool = False):
    """The transfer matrix (dsim_region_transfer_matrix): the attention mass every image of set B sends into every set-A image's
    weighted tokens.  fa, fb: (q, k) or (q, k, v) tuples of [n][B][N][H*D] device tensors of one dtype and geometry (v is not read);
    weights_a: uint8 cuda (n_a, N), token t of A_i weighs byte / 255.  Returns f32 (n_a, n_b, N): cell (i, j) is
    ``pair_region_transfer(..., directions=2)[p, 1]`` of the pair (a = fa[i], b = fb[j]) -- fb[j]'s queries over fa[i]'s keys and
    weights, on fb[j]'s grid -- bit for bit, in one launch.  return_status: also an int32 (n_a, n_b) tensor, 1 where a cell has a
    non-finite probability."""
    (qa, ka), (qb, kb) = fa[:2], fb[:2]
    ok = ka.shape == qa.shape and kb.shape == qb.shape and qa.shape[1:] == qb.shape[1:]
    B, N, D = _check_features((qa, ka, qb, kb), heads, ok, _SETS_MSGS)
    n_a, n_b, dev, dt = qa.shape[0], qb.shape[0], qa.device, _TORCH2DSIM[qa.dtype]
    weights_a = _token_rows(_WEIGHTS, weights_a, n_a, N, "the token weights weights_a", "n_a")
    _require_cuda(qa, ka, qb, kb, weights_a)
    mass = torch.empty((n_a, n_b, N), dtype=torch.float32, device=dev)
    status = _i32((n_a, n_b), dev, return_status)
    _tail_call(dev, "region_transfer_matrix", (n_a, n_b, B, heads, N, D, dt),
               f"no transfer matrix for n_a={n_a} n_b={n_b} B={B} H={heads} N={N} D={D}", qa.data_ptr(), ka.data_ptr(),
               weights_a.data_ptr(), n_a, qb.data_ptr(), kb.data_ptr(), n_b, B, heads, N, D, dt, mass.data_ptr(), _ptr(status))
    return (mass, status) if return_status else mass


def score_matrix_workspace_bytes(n_a: int, n_b: int, B: int, heads: int, N: int, D: int, dtype: torch.dtype) -> int:
    return int(_lib.lib().dsim_score_matrix_workspace_bytes(n_a, n_b, B, heads, N, D, _TORCH2DSIM[dtype]))


def score_matrix_regions_workspace_bytes(n_a: int, n_b: int, B: int, heads: int, N: int, D: int, dtype: torch.dtype) -> int:
    return int(_lib.lib().dsim_score_matrix_regions_workspace_bytes(n_a, n_b, B, heads, N, D, _TORCH2DSIM[dtype]))


def score_matrix_weights_workspace_bytes(n_a: int, n_b: int, B: int, heads: int, N: int, D: int, dtype: torch.dtype) -> int:
    return int(_lib.lib().dsim_score_matrix_weights_workspace_bytes(n_a, n_b, B, heads, N, D, _TORCH2DSIM.get(dtype, -1)))


def score_matrix_cell_regions_workspace_bytes(n_a: int, n_b: int, B: int, heads: int, N: int, D: int, dtype: torch.dtype) -> int:
    return int(_lib.lib().dsim_score_matrix_cell_regions_workspace_bytes(n_a, n_b, B, heads, N, D, _TORCH2DSIM.get(dtype, -1)))


def score_matrix_cell_weights_workspace_bytes(n_a: int, n_b: int, B: int, heads: int, N: int, D: int, dtype: torch.dtype) -> int:
    return int(_lib.lib().dsim_score_matrix_cell_weights_workspace_bytes(n_a, n_b, B, heads, N, D, _TORCH2DSIM.get(dtype, -1)))


def _score_matrix(fa, fb, heads, similarity, return_status, region=None, return_extra=False, cells: bool = False):
    """score_matrix and its two region forms; region: (_TokenRows, set A's rows, set B's rows); cells: set B's rows are
    (n_a, n_b, N), one per cell (the cell-region forms)"""
    sim = _similarity_code(similarity)
    if region is None:
        _require_cuda(*fa, *fb)
    (qa, ka, va, qb, kb, vb), B, N, D = _check_two_sets(fa, fb, heads)
    n_a, n_b, dev, dt = qa.shape[0], qb.shape[0], qa.device, _TORCH2DSIM[qa.dtype]
    name, noun, rows_a, rows_b = "score_matrix", "score matrix", (), ()
    if region is not None:
        form, rows_a, rows_b = region
        rows_a = _token_rows(form, rows_a, n_a, N, f"{form.what} {form.arg}_a", "n")
        if cells:
            if rows_b.ndim != 3:
                raise _lib.DsimError(f"{form.what} {form.arg}_b_cells must be (n_a, n_b, N) = ({n_a}, {n_b}, {N}): {tuple(rows_b.shape)}")
            rows_b = _token_rows(form, rows_b, (n_a, n_b), N, f"{form.what} {form.arg}_b_cells", "n_a, n_b")
        else:
            rows_b = _token_rows(form, rows_b, n_b, N, f"{form.what} {form.arg}_b", "n")
        _require_cuda(qa, ka, va, qb, kb, vb, rows_a, rows_b)          # (after the shape checks: those need no device)
        name, noun = f"score_matrix_{'cell_' if cells else ''}{form.suffix}", ("cell-" if cells else "") + form.matrix
        rows_a, rows_b = (rows_a.data_ptr(),), (rows_b.data_ptr(),)
    out = torch.empty((n_a, n_b), dtype=torch.float32, device=dev)
    status = _i32((n_a, n_b), dev, return_status)
    extra = _i32(n_a + (n_a * n_b if cells else n_b), dev, return_extra)
    _tail_call(dev, name, (n_a, n_b, B, heads, N, D, dt), f"no {noun} for n_a={n_a} n_b={n_b} B={B} H={heads} N={N} D={D}", qa.data_ptr(),
               ka.data_ptr(), va.data_ptr(), *rows_a, n_a, qb.data_ptr(), kb.data_ptr(), vb.data_ptr(), *rows_b, n_b, B, heads, N, D, dt,
               sim, out.data_ptr(), _ptr(status), *(() if region is None else (_ptr(extra),)))
    return _with_extras(out, status, extra)


def score_matrix(fa, fb, heads: int, similarity: str = "cosine", return_status: bool = False):
    """Every image of set A against every image of set B (dsim_score_matrix).  fa, fb: (q, k, v) tuples of [n][B][N][H*D]
    device tensors of one dtype.  Returns the (n_a, n_b) f32 device tensor whose cell (i, j) is pair_score of (fa[i], fb[j]);
    each image's self-attention is computed once.  return_status: also an int32 (n_a, n_b) tensor, 1 where the score is
    NaN / infinite."""
    return _score_matrix(fa, fb, heads, similarity, return_status)


def score_matrix_regions(fa, fb, mask_a: torch.Tensor, mask_b: torch.Tensor, heads: int, similarity: str = "cosine",
                         return_status: bool = False, return_counts: bool = False):
    """Every image of set A over its region against every image of set B over its region (dsim_score_matrix_regions).  fa, fb:
    (q, k, v) tuples of [n][B][N][H*D] device tensors of one dtype; mask_a (n_a, N), mask_b (n_b, N): bool or uint8 cuda, non-zero =
    the token is in its image's region.  Returns the (n_a, n_b) f32 device tensor whose cell (i, j) is pair_score_regions of
    (fa[i] over mask_a[i], fb[j] over mask_b[j]); each image's self-attention over its region is computed once.  return_status:
    also an int32 (n_a, n_b) tensor, 1 where the score is NaN / infinite, 2 where a region of the cell is empty (score NaN);
    return_counts: also the int32 (n_a + n_b,) region sizes, set A's then set B's."""
    return _score_matrix(fa, fb, heads, similarity, return_status, (_MASKS, mask_a, mask_b), return_counts)


def score_matrix_weights(fa, fb, weights_a: torch.Tensor, weights_b: torch.Tensor, heads: int, similarity: str = "cosine",
                         return_status: bool = False, return_sums: bool = False):
    """The soft score matrix (dsim_score_matrix_weights): score_matrix_regions with a weight per token instead of a bit.  fa, fb:
    (q, k, v) tuples of [n][B][N][H*D] device tensors of one dtype; weights_a (n_a, N), weights_b (n_b, N): uint8 cuda, token t of
    an image weighs byte / 255.  Returns the (n_a, n_b) f32 device tensor whose cell (i, j) is pair_score_weights of (fa[i] under
    weights_a[i], fb[j] under weights_b[j]), bit for bit; each image's self-attention is computed once.  return_status: also an
    int32 (n_a, n_b) tensor, 1 where the score is NaN / infinite, 2 where an image of the cell has no weight at all (score NaN);
    return_sums: also the int32 (n_a + n_b,) byte sums, set A's then set B's."""
    return _score_matrix(fa, fb, heads, similarity, return_status, (_WEIGHTS, weights_a, weights_b), return_sums)


def score_matrix_cell_regions(fa, fb, mask_a: torch.Tensor, mask_b_cells: torch.Tensor, heads: int, similarity: str = "cosine",
                              return_status: bool = False, return_counts: bool = False):
    """The cell-region score matrix (dsim_score_matrix_cell_regions): score_matrix_regions with set B's masks per CELL.  fa, fb,
    mask_a (n_a, N): as score_matrix_regions; mask_b_cells (n_a, n_b, N): bool or uint8 cuda, row [i][j] is fb[j]'s region against
    query i.  Returns the (n_a, n_b) f32 device tensor whose cell (i, j) is pair_score_regions of (fa[i] over mask_a[i], fb[j] over
    mask_b_cells[i][j]), bit for bit; fa[i]'s self-attention over its region is computed once, a cell costs three attentions.
    return_status: also an int32 (n_a, n_b) tensor, 1 where the score is NaN / infinite, 2 where a region of the cell is empty
    (score NaN); return_counts: also the int32 (n_a + n_a n_b,) region sizes, set A's then the cells' in cell order."""
    return _score_matrix(fa, fb, heads, similarity, return_status, (_MASKS, mask_a, mask_b_cells), return_counts, cells=True)


def score_matrix_cell_weights(fa, fb, weights_a: torch.Tensor, weights_b_cells: torch.Tensor, heads: int, similarity: str = "cosine",
                              return_status: bool = False, return_sums: bool = False):
    """The soft cell-region score matrix (dsim_score_matrix_cell_weights): score_matrix_weights with set B's weights per CELL,
    weights_b_cells uint8 cuda (n_a, n_b, N).  Cell (i, j) is pair_score_weights of (fa[i] under weights_a[i], fb[j] under
    weights_b_cells[i][j]), bit for bit.  return_status: as score_matrix_weights; return_sums: also the int32 (n_a + n_a n_b,) byte
    sums, set A's then the cells' in cell order."""
    return _score_matrix(fa, fb, heads, similarity, return_status, (_WEIGHTS, weights_a, weights_b_cells), return_sums, cells=True)


# ---- feature-cosine metrics (diffeats, dinofeats): the tapped self-attention's own output, its pair cosine and Gram matrix -------
_FEAT_IMAGES = 65535                 # dsim_attn_features carries the images on a grid axis: more are chunked
_FEAT_PAIRS = 65535                  # ... and dsim_feature_pair_score the pairs
_FEAT_BYTES = (1 << 31) - 1          # one call's projection slab stays under 2 GiB


def attn_features_workspace_bytes(n: int, B: int, heads: int, N: int, D: int, dtype: torch.dtype, proj: bool) -> int:
    return int(_lib.lib().dsim_attn_features_workspace_bytes(n, B, heads, N, D, B * N * heads * D, _TORCH2DSIM.get(dtype, -1), int(proj)))


def attn_features(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, heads: int, w_out: Optional[torch.Tensor] = None,
                  bias: Optional[torch.Tensor] = None, minmax: bool = False):
    """The tapped self-attention's own output per image (dsim_attn_features).  q,k,v: contiguous [n][B][N][H*D] of one shape.
    w_out / bias (both or neither): the layer's output projection, [C][C] in the features' dtype and f32 [C], C = H*D.  minmax:
    min-max normalise each image over all its values (metrics/diffeats.py:136-140).  Returns (feats [n][B][N][C] in q's dtype,
    stats f32 [n][4] = sum of squares, min, max, 0); an image's rows do not depend on the other images."""
    _require_cuda(q, k, v, *(t for t in (w_out, bias) if t is not None))
    B, N, D = _check_features((q, k, v), heads, k.shape == q.shape == v.shape, _PAIR_MSGS)
    Cc, n, dt = heads * D, q.shape[0], _TORCH2DSIM[q.dtype]
    if (w_out is None) != (bias is None):
        raise _lib.DsimError("w_out and bias come together")
    if w_out is not None and (w_out.dtype != q.dtype or tuple(w_out.shape) != (Cc, Cc) or bias.dtype != torch.float32
                              or tuple(bias.shape) != (Cc,) or not (w_out.is_contiguous() and bias.is_contiguous())):
        raise _lib.DsimError(f"w_out must be contiguous {q.dtype} ({Cc}, {Cc}) and bias float32 ({Cc},)")
    L = B * N * Cc
    feats = torch.empty_like(q)
    stats = torch.empty((n, 4), dtype=torch.float32, device=q.device)
    step = max(1, min(_FEAT_IMAGES, _FEAT_BYTES // (L * q.element_size())))
    for i0 in range(0, n, step):
        m = min(step, n - i0)
        sl = slice(i0, i0 + m)
        _tail_call(q.device, "attn_features", (m, B, heads, N, D, L, dt, int(w_out is not None)),
                   f"no attention features for n={m} B={B} H={heads} N={N} D={D}", q[sl].data_ptr(), k[sl].data_ptr(), v[sl].data_ptr(),
                   m, B, heads, N, D, L, dt, _ptr(w_out), _ptr(bias), int(bool(minmax)), feats[sl].data_ptr(), stats[sl].data_ptr())
    return feats, stats


def _check_feats(feats: torch.Tensor, stats: torch.Tensor, what: str = "feats") -> int:
    """attn_features' outputs as the consumers take them: [n][...] contiguous of the three dtypes, f32 [n][4]; the image length L"""
    if feats.dtype not in _TORCH2DSIM or feats.ndim < 2 or not feats.is_contiguous():
        raise _lib.DsimError(f"{what} must be contiguous [n][...] of dtype float32, bfloat16 or float16")
    if stats.dtype != torch.float32 or tuple(stats.shape) != (feats.shape[0], 4) or not stats.is_contiguous():
        raise _lib.DsimError(f"the stats of {what} must be contiguous float32 ({feats.shape[0]}, 4)")
    return feats[0].numel()


def feature_pair_score_workspace_bytes(n_pairs: int, L: int, dtype: torch.dtype) -> int:
    return int(_lib.lib().dsim_feature_pair_score_workspace_bytes(n_pairs, L, _TORCH2DSIM.get(dtype, -1)))


def feature_pair_score(feats: torch.Tensor, stats: torch.Tensor, idx_a: torch.Tensor, idx_b: torch.Tensor, return_status: bool = False):
    """The cosine of the flattened features of images idx_a[p] and idx_b[p] (dsim_feature_pair_score), eps 1e-8.  feats, stats:
    attn_features' outputs; idx: contiguous int32 cuda [n_pairs].  return_status: also an int32 [n_pairs] tensor, 1 where the score
    is NaN / infinite."""
    _require_cuda(feats, stats, idx_a, idx_b)
    L = _check_feats(feats, stats)
    if idx_a.dtype != torch.int32 or idx_b.dtype != torch.int32 or idx_a.numel() != idx_b.numel():
        raise _lib.DsimError("pair indices must be int32 and of one length")
    if not (idx_a.is_contiguous() and idx_b.is_contiguous()):
        raise _lib.DsimError("features and indices must be contiguous")
    n_pairs, dt = idx_a.numel(), _TORCH2DSIM[feats.dtype]
    out = torch.empty(n_pairs, dtype=torch.float32, device=feats.device)
    status = _i32(n_pairs, feats.device, return_status)
    for i0 in range(0, n_pairs, _FEAT_PAIRS):
        m = min(_FEAT_PAIRS, n_pairs - i0)
        sl = slice(i0, i0 + m)
        _tail_call(feats.device, "feature_pair_score", (m, L, dt), f"no feature pair score for n_pairs={m} L={L}", feats.data_ptr(),
                   stats.data_ptr(), idx_a[sl].data_ptr(), idx_b[sl].data_ptr(), m, L, dt, out[sl].data_ptr(),
                   _ptr(None if status is None else status[sl]))
    return (out, status) if return_status else out


def feature_matrix_workspace_bytes(n_a: int, n_b: int, L: int, dtype: torch.dtype) -> int:
    return int(_lib.lib().dsim_feature_matrix_workspace_bytes(n_a, n_b, L, _TORCH2DSIM.get(dtype, -1)))


def feature_matrix(fa, fb, return_status: bool = False, k_chunk: Optional[int] = None):
    """Every image of set A against every image of set B (dsim_feature_matrix; k_chunk: dsim_feature_matrix_chunked, the f32 partial
    sums ending every k_chunk elements -- for long descriptors of one sign).  fa, fb: (feats, stats) of attn_features, one
    dtype and image length.  Returns the (n_a, n_b) f32 device tensor of cosines; a cell depends on its two images alone and is
    close to, not bit-equal to, feature_pair_score of them.  return_status: also an int32 (n_a, n_b) tensor, 1 where NaN / infinite."""
    (xa, sa), (xb, sb) = fa, fb
    _require_cuda(xa, sa, xb, sb)
    L = _check_feats(xa, sa, "set A's feats")
    if _check_feats(xb, sb, "set B's feats") != L or xb.dtype != xa.dtype:
        raise _lib.DsimError("both sets' features must share dtype and image length")
    n_a, n_b, dt = xa.shape[0], xb.shape[0], _TORCH2DSIM[xa.dtype]
    out = torch.empty((n_a, n_b), dtype=torch.float32, device=xa.device)
    status = _i32((n_a, n_b), xa.device, return_status)
    if k_chunk is not None:
        _tail_call(xa.device, "feature_matrix_chunked", (n_a, n_b, L, dt, int(k_chunk)),
                   f"no feature matrix for n_a={n_a} n_b={n_b} L={L} k_chunk={k_chunk}", xa.data_ptr(), sa.data_ptr(), n_a, xb.data_ptr(),
                   sb.data_ptr(), n_b, L, dt, int(k_chunk), out.data_ptr(), _ptr(status))
        return _with_extras(out, status)
    _tail_call(xa.device, "feature_matrix", (n_a, n_b, L, dt), f"no feature matrix for n_a={n_a} n_b={n_b} L={L}", xa.data_ptr(),
               sa.data_ptr(), n_a, xb.data_ptr(), sb.data_ptr(), n_b, L, dt, out.data_ptr(), _ptr(status))
    return _with_extras(out, status)


# ---- single-operator entry points (kernel-level parity tests) -----------------------------------
def op_linear(x, w, bias=None, residual=None, geglu=False):
    L = _lib.lib()
    _require_cuda(x, w, bias, residual)
    M, K = x.shape
    N = w.shape[0] // 2 if geglu else w.shape[0]
    out = torch.empty((M, N), dtype=x.dtype, device=x.device)
    _lib.check(L.dsim_op_linear(x.data_ptr(), w.data_ptr(), _ptr(bias), _ptr(residual), out.data_ptr(), M, N, K,
                                _TORCH2DSIM[x.dtype], int(geglu), _stream_ptr()), "op_linear")
    return out


def op_ff_fused(x, ln_g, ln_b, w1, b1, w2, b2, eps=1e-5):
    """x + ff.net.2(GEGLU(ff.net.0.proj(LayerNorm(x)))) in one launch (bf16, or fp16: the twin kernel; C = 320); w1 [8C][C],
    w2 [C][4C] f32."""
    L = _lib.lib()
    _require_cuda(x, ln_g, ln_b, w1, b1, w2, b2)
    if x.dtype not in (torch.bfloat16, torch.float16):
        raise TypeError("op_ff_fused takes a torch.bfloat16 or torch.float16 input")
    M, Cc = x.shape
    out = torch.empty_like(x)
    _lib.check(L.dsim_op_ff_fused_dt(x.data_ptr(), ln_g.data_ptr(), ln_b.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(),
                                     b2.data_ptr(), out.data_ptr(), M, Cc, float(eps), _TORCH2DSIM[x.dtype], _stream_ptr()),
               "op_ff_fused")
    return out


def op_ln_linear(x, ln_g, ln_b, w, eps=1e-5):
    """LayerNorm(x) W^T in one launch (bf16, or fp16: the twin kernel; C = 320 or 640, bias-free, N a multiple of 64 up to 3 C);
    w [N][C] f32; ln_g = ln_b = None skips the LayerNorm."""
    L = _lib.lib()
    _require_cuda(x, ln_g, ln_b, w)
    if x.dtype not in (torch.bfloat16, torch.float16):
        raise TypeError("op_ln_linear takes a torch.bfloat16 or torch.float16 input")
    M, Cc = x.shape
    N = w.shape[0]
    out = torch.empty((M, N), dtype=x.dtype, device=x.device)
    _lib.check(L.dsim_op_ln_linear_dt(x.data_ptr(), _ptr(ln_g), _ptr(ln_b), w.data_ptr(), out.data_ptr(), M, Cc, N, float(eps),
                                      _TORCH2DSIM[x.dtype], _stream_ptr()), "op_ln_linear")
    return out


def op_gn_linear(x, gamma, beta, groups, w, bias=None, eps=1e-6):
    """GroupNorm(x [B][HW][C]) W^T + bias as a statistics pass and one row-resident launch (16-bit dtypes; C = 320 or 640, N a
    multiple of 64 up to C, HW % 128 == 0); w [N][C] f32, bias [N] f32 or None; gamma = beta = None: no normalisation."""
    L = _lib.lib()
    _require_cuda(x, gamma, beta, w, bias)
    if x.dtype not in (torch.bfloat16, torch.float16):
        raise TypeError("op_gn_linear takes a torch.bfloat16 or torch.float16 input")
    B, HW, Cc = x.shape
    N = w.shape[0]
    out = torch.empty((B, HW, N), dtype=x.dtype, device=x.device)
    _lib.check(L.dsim_op_gn_linear_dt(x.data_ptr(), _ptr(gamma), _ptr(beta), int(groups), float(eps), w.data_ptr(), _ptr(bias),
                                      out.data_ptr(), B, HW, Cc, N, _TORCH2DSIM[x.dtype], _stream_ptr()), "op_gn_linear")
    return out


def op_conv3x3(x, w, bias=None, residual=None, stride=1, upsample=False):
    """x: [B][H][W][Cin] token-major; w: [Cout][Cin][3][3] f32."""
    L = _lib.lib()
    _require_cuda(x, w, bias, residual)
    B, H, W, Cin = x.shape
    Cout = w.shape[0]
    Ho, Wo = (2 * H, 2 * W) if upsample else (((H + 1) // 2, (W + 1) // 2) if stride == 2 else (H, W))      # ceil: odd sides (as the executor)
    out = torch.empty((B, Ho, Wo, Cout), dtype=x.dtype, device=x.device)
    _lib.check(L.dsim_op_conv3x3(x.data_ptr(), w.data_ptr(), _ptr(bias), _ptr(residual), out.data_ptr(), B, H, W, Cin,
                                 Cout, stride, int(upsample), _TORCH2DSIM[x.dtype], _stream_ptr()), "op_conv3x3")
    return out


_GEMM_EPI = {"none": 0, "residual": 1, "geglu": 2}
_GEMM_EK = ("plain", "residual", "dit", "act", "plain_gn", "residual_gn")


def op_gemm(a0, w, out, *, a1=None, conv=None, bias=None, bias2=None, rows_per_batch=0, act=0, gate=None, gate2=None,
            epi="none", residual=None, ldo=None, out_split=0, out_split_stride=0, force_big=False, wb_rows=0, wb_stride=0,
            gn_part=None, gn_hw=0):
    """The implicit GEMM with its whole epilogue surface as one operator (dsim_op_gemm).  Returns the launch record: the
    instantiation that ran (bm, bn, kind "linear" / "conv3" / "conv3p", geglu, ek, small) and gemm_family()'s name for it.

    linear: a0 [M][C0] (a1 [M][C1]: the K concatenation), w f32 [N][K] ([M / wb_rows][N][K] with wb_rows);
    conv:   a0 [B][H][W][C0], conv = dict(stride=1|2, ups=0|1, pad=1|0), w f32 [N][C0][3][3].
    N counts weight rows (GEGLU: [h ; g], 2 x the output columns).  out / residual: tensors of the compute dtype whose storage
    holds M rows of ldo elements (out_split: N / out_split such outputs, out_split_stride BYTES apart, from out's first element).
    bias / bias2 / gate / gate2: f32 [N] (gate: [output columns]); gn_part: f32 [M / gn_hw][gn_hw / 64][N / 4][2]."""
    L = _lib.lib()
    _require_cuda(a0, a1, w, out, bias, bias2, gate, gate2, residual, gn_part)
    if a0.dtype not in _TORCH2DSIM:
        raise _lib.DsimError("a0 must be float32, bfloat16 or float16")
    dt = a0.dtype
    for t, nm in ((a1, "a1"), (out, "out"), (residual, "residual")):
        if t is not None and t.dtype != dt:
            raise _lib.DsimError(f"{nm} must have a0's dtype {dt}")
    for t, nm in ((w, "w"), (bias, "bias"), (bias2, "bias2"), (gate, "gate"), (gate2, "gate2"), (gn_part, "gn_part")):
        if t is not None and t.dtype != torch.float32:
            raise _lib.DsimError(f"{nm} must be float32")
    if epi not in _GEMM_EPI:
        raise ValueError(epi)
    op = _lib.GemmOpC()
    if conv is None:
        if a0.ndim != 2 or (a1 is not None and (a1.ndim != 2 or a1.shape[0] != a0.shape[0])):
            raise _lib.DsimError("linear: a0 [M][C0], a1 [M][C1]")
        M, C0 = a0.shape
        C1 = 0 if a1 is None else a1.shape[1]
        K = C0 + C1
        if w.shape[-1] != K or w.ndim != (3 if wb_rows else 2) or (wb_rows and w.shape[0] * wb_rows != M):
            raise _lib.DsimError("linear: w must be [N][K] (with wb_rows: [M / wb_rows][N][K])")
        N = w.shape[-2]
        op.mode = 0
    else:
        if a0.ndim != 4 or a1 is not None or wb_rows or w.ndim != 4 or w.shape[1:] != (a0.shape[3], 3, 3):
            raise _lib.DsimError("conv: a0 [B][H][W][C0], w [N][C0][3][3], no a1 / wb_rows")
        B, H, W, C0 = a0.shape
        stride, ups, pad = int(conv.get("stride", 1)), int(conv.get("ups", 0)), int(conv.get("pad", 1))
        Ho = 2 * H if ups else ((H + 1) // 2 if pad else H // 2) if stride == 2 else H
        Wo = 2 * W if ups else ((W + 1) // 2 if pad else W // 2) if stride == 2 else W
        M, N, K, C1 = B * Ho * Wo, w.shape[0], 9 * C0, 0
        op.mode, op.H, op.W, op.stride, op.ups, op.pad = 1, H, W, stride, ups, pad
    ncol = N // 2 if epi == "geglu" else N
    ldo = ncol if ldo is None else int(ldo)
    es = out.element_size()
    nout = N // out_split if out_split else 1
    need = (nout - 1) * int(out_split_stride) + M * ldo * es
    if ldo < (out_split or ncol) or out.numel() * es < need:
        raise _lib.DsimError(f"out holds {out.numel() * es} bytes, the launch writes up to {need}")
    if residual is not None and residual.numel() < M * ldo:
        raise _lib.DsimError("residual must hold M rows of ldo elements")
    for t, nm, n in ((bias, "bias", N), (bias2, "bias2", N), (gate, "gate", ncol), (gate2, "gate2", ncol)):
        if t is not None and t.numel() != n:
            raise _lib.DsimError(f"{nm} must have {n} elements")
    if gn_part is not None and (gn_hw <= 0 or M % gn_hw or gn_part.numel() != (M // gn_hw) * (gn_hw // 64) * (N // 4) * 2):
        raise _lib.DsimError("gn_part must be f32 [M / gn_hw][gn_hw / 64][N / 4][2]")
    op.A0, op.C0, op.A1, op.C1 = a0.data_ptr(), C0, _ptr(a1), C1
    op.M, op.N, op.K = M, N, K
    op.w, op.wb_rows, op.wb_stride = w.data_ptr(), int(wb_rows), int(wb_stride)
    op.bias, op.bias2, op.rows_per_batch = _ptr(bias), _ptr(bias2), int(rows_per_batch)
    op.act, op.gate, op.gate2 = int(act), _ptr(gate), _ptr(gate2)
    op.epi, op.residual, op.out, op.ldo = _GEMM_EPI[epi], _ptr(residual), out.data_ptr(), ldo
    op.out_split, op.out_split_stride, op.force_big = int(out_split), int(out_split_stride), int(bool(force_big))
    op.gn_part, op.gn_hw, op.dtype = _ptr(gn_part), int(gn_hw), _TORCH2DSIM[dt]
    rec = _lib.GemmLaunchC()
    with torch.cuda.device(a0.device):
        _lib.check(L.dsim_op_gemm(C.byref(op), C.byref(rec), _stream_ptr()), "op_gemm")
    return {"bm": rec.bm, "bn": rec.bn, "kind": ("linear", "conv3", "conv3p")[rec.kind], "geglu": bool(rec.geglu),
            "ek": _GEMM_EK[rec.ek], "small": bool(rec.small), "family": rec.family.decode()}


def op_groupnorm_pre(x, gamma, beta, groups, eps, silu, part32, chunks):
    """GroupNorm (+ SiLU) of x [B][HW][C] with its statistics from a conv epilogue's gn_part (part32 f32 [B][chunks][C / 4][2])."""
    L = _lib.lib()
    _require_cuda(x, gamma, beta, part32)
    if x.dtype not in (torch.bfloat16, torch.float16):
        raise _lib.DsimError("op_groupnorm_pre takes a 16-bit input (the statistics epilogue is 16-bit only)")
    B, HW, Cc = x.shape
    if part32.dtype != torch.float32 or part32.numel() != B * chunks * (Cc // 4) * 2:
        raise _lib.DsimError("part32 must be f32 [B][chunks][C / 4][2]")
    if gamma.numel() != Cc or beta.numel() != Cc:
        raise _lib.DsimError("gamma / beta must have C elements")
    out = torch.empty_like(x)
    _lib.check(L.dsim_op_groupnorm_pre(x.data_ptr(), Cc, gamma.data_ptr(), beta.data_ptr(), out.data_ptr(), B, HW, groups, float(eps),
                                       int(silu), _TORCH2DSIM[x.dtype], part32.data_ptr(), int(chunks), _stream_ptr()),
               "op_groupnorm_pre")
    return out


def op_groupnorm(x0, x1, gamma, beta, groups, eps, silu):
    """x0: [B][HW][C0], x1: optional [B][HW][C1] (channel concat)."""
    L = _lib.lib()
    _require_cuda(x0, x1, gamma, beta)
    B, HW, C0 = x0.shape
    C1 = 0 if x1 is None else x1.shape[2]
    out = torch.empty((B, HW, C0 + C1), dtype=x0.dtype, device=x0.device)
    _lib.check(L.dsim_op_groupnorm(x0.data_ptr(), C0, _ptr(x1), C1, gamma.data_ptr(), beta.data_ptr(), out.data_ptr(),
                                   B, HW, groups, float(eps), int(silu), _TORCH2DSIM[x0.dtype], _stream_ptr()),
               "op_groupnorm")
    return out


def op_layernorm(x, gamma, beta, eps=1e-5):
    L = _lib.lib()
    _require_cuda(x, gamma, beta)
    M, Cc = x.shape
    out = torch.empty_like(x)
    _lib.check(L.dsim_op_layernorm(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), out.data_ptr(), M, Cc, float(eps),
                                   _TORCH2DSIM[x.dtype], _stream_ptr()), "op_layernorm")
    return out


def op_layernorm_mod(x, scale2, shift2, rows_per_batch, eps=1e-6, out=None):
    """LayerNorm without affine, then y = xhat * (1 + scale2[half]) + shift2[half], half = (row // rows_per_batch) & 1 (DiT's adaLN
    modulation); x [M][C], scale2 / shift2 f32 [2][C].  out: None (a new tensor) or a tensor to write (x itself: in place)."""
    L = _lib.lib()
    _require_cuda(x, scale2, shift2, out)
    M, Cc = x.shape
    for t, nm in ((scale2, "scale2"), (shift2, "shift2")):
        if t.dtype != torch.float32 or t.numel() != 2 * Cc:
            raise _lib.DsimError(f"{nm} must be f32 [2][C]")
    out = torch.empty_like(x) if out is None else out
    _lib.check(L.dsim_op_layernorm_mod(x.data_ptr(), scale2.data_ptr(), shift2.data_ptr(), out.data_ptr(), M, Cc, int(rows_per_batch),
                                       float(eps), _TORCH2DSIM[x.dtype], _stream_ptr()), "op_layernorm_mod")
    return out


# ---- the kernels in front of the models (csrc/pack.hip, the patch embedding, the VAE's fold and transpose), one operator each.
# `out`: None (a new tensor) or the tensor to write -- the tests hand in a view of a sentinel-filled buffer they own.
def _out(out, shape, dtype, device):
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    _require_cuda(out)
    if out.dtype != dtype or out.numel() != math.prod(shape):
        raise _lib.DsimError(f"out must hold {tuple(shape)} elements of {dtype}")
    return out


def _f32(*named):
    for t, nm in named:
        if t is not None and t.dtype != torch.float32:
            raise _lib.DsimError(f"{nm} must be float32")


def op_conv_in(lat, noise, sa, sb, w, bias, dtype, dup=1, force=0, gn_part=None, out=None):
    """Noising + CFG copies + conv_in (dsim_op_conv_in): lat / noise f32 [n][Cin][S][S] (noise None: no noising), w f32
    [Cout][Cin][3][3], bias f32 [Cout] -> ([n * dup][S * S][Cout] in dtype, the kernel that ran: "generic" / "eight" / "rows").
    force: 0 the executors' choice, or 1 / 2 / 3 = that kernel; gn_part: f32 [n][S * S / 64][Cout / 4][2] to fill (row kernel)."""
    L = _lib.lib()
    _require_cuda(lat, noise, w, bias, gn_part)
    _f32((lat, "lat"), (noise, "noise"), (w, "w"), (bias, "bias"), (gn_part, "gn_part"))
    n, Cin, S, S2 = lat.shape
    Cout = w.shape[0]
    if S != S2 or tuple(w.shape) != (Cout, Cin, 3, 3) or bias.numel() != Cout or (noise is not None and noise.shape != lat.shape):
        raise _lib.DsimError("conv_in: lat / noise [n][Cin][S][S], w [Cout][Cin][3][3], bias [Cout]")
    if gn_part is not None and (S * S % 64 or Cout % 4 or gn_part.numel() != n * (S * S // 64) * (Cout // 4) * 2):
        raise _lib.DsimError("gn_part must be f32 [n][S * S / 64][Cout / 4][2]")
    out = _out(out, (n * dup, S * S, Cout), dtype, lat.device)
    kernel = C.c_int(0)
    with torch.cuda.device(lat.device):
        _lib.check(L.dsim_op_conv_in(lat.data_ptr(), _ptr(noise), float(sa), float(sb), w.data_ptr(), bias.data_ptr(), out.data_ptr(),
                                     _TORCH2DSIM[dtype], n, Cin, S, Cout, int(dup), _ptr(gn_part), int(force), C.byref(kernel),
                                     _stream_ptr()), "op_conv_in")
    return out.view(n * dup, S * S, Cout), _lib.CONV_IN_KERNELS[kernel.value]


def op_timestep_sincos(dim, t, out=None, device="cuda"):
    """diffusers Timesteps(dim, flip_sin_to_cos=True, downscale_freq_shift=0) of the integer t -> f32 [dim] = [cos | sin]"""
    out = _out(out, (dim,), torch.float32, device)
    with torch.cuda.device(out.device):
        _lib.check(_lib.lib().dsim_op_timestep_sincos(out.data_ptr(), int(dim), int(t), _stream_ptr()), "op_timestep_sincos")
    return out


def op_sincos_values(dim, vals, out=None):
    """the same embedding of each of the f32 values vals [count] -> f32 [count][dim]"""
    _require_cuda(vals)
    _f32((vals, "vals"))
    out = _out(out, (vals.numel(), dim), torch.float32, vals.device)
    with torch.cuda.device(vals.device):
        _lib.check(_lib.lib().dsim_op_sincos_values(out.data_ptr(), int(dim), vals.data_ptr(), vals.numel(), _stream_ptr()),
                   "op_sincos_values")
    return out.view(vals.numel(), dim)


def op_gemv_f32(W, bias, x, act=0, out=None):
    """y = W act(x) + bias in f32: W [N][K] in any of the three dtypes, bias None or [N] in any, x f32 [K]; act 1: SiLU on x"""
    _require_cuda(W, bias, x)
    _f32((x, "x"))
    N, K = W.shape
    if x.numel() != K or (bias is not None and bias.numel() != N):
        raise _lib.DsimError("gemv: W [N][K], x [K], bias [N]")
    out = _out(out, (N,), torch.float32, W.device)
    with torch.cuda.device(W.device):
        _lib.check(_lib.lib().dsim_op_gemv_f32(W.data_ptr(), _TORCH2DSIM[W.dtype], _ptr(bias), _TORCH2DSIM[bias.dtype] if bias is not None else 0,
                                               x.data_ptr(), out.data_ptr(), N, K, int(act), _stream_ptr()), "op_gemv_f32")
    return out


def op_pack(kind, src, dst_dtype, geglu=0, out=None):
    """One weight pack (dsim_op_pack): kind "linear" (src [N][K]), "conv3" / "conv_in" (src [Cout][Cin][3][3]), "vector" (src [N]);
    src in any of the three dtypes -> the packed tensor in dst_dtype (conv_in [9 Cin][Cout] and vector: float32 only)."""
    _require_cuda(src)
    k = _lib.PACK_KINDS.index(kind)
    rows, cols = src.shape[0], (src.shape[1] if src.ndim > 1 else 1)
    if src.ndim != {"linear": 2, "conv3": 4, "conv_in": 4, "vector": 1}[kind] or (src.ndim == 4 and tuple(src.shape[2:]) != (3, 3)):
        raise _lib.DsimError(f"pack {kind}: wrong source shape {tuple(src.shape)}")
    shape = {"linear": (rows, cols), "conv3": (rows, 9, cols), "conv_in": (9 * cols, rows), "vector": (rows,)}[kind]
    out = _out(out, shape, dst_dtype, src.device)
    with torch.cuda.device(src.device):
        _lib.check(_lib.lib().dsim_op_pack(k, src.data_ptr(), _TORCH2DSIM[src.dtype], out.data_ptr(), _TORCH2DSIM[dst_dtype], rows, cols,
                                           int(geglu), _stream_ptr()), "op_pack")
    return out.view(shape)


def op_dup_batch(x, out=None):
    """[n][...] -> [2 n][...]: every batch element twice in a row (an element's bytes must be a multiple of 16)"""
    _require_cuda(x)
    n = x.shape[0]
    out = _out(out, (2 * n,) + tuple(x.shape[1:]), x.dtype, x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().dsim_op_dup_batch(x.data_ptr(), out.data_ptr(), n, x[0].numel() * x.element_size(), _stream_ptr()),
                   "op_dup_batch")
    return out.view((2 * n,) + tuple(x.shape[1:]))


def op_resize_nearest(x, Hout, Wout, out=None):
    """token-major nearest resize [B][Hin][Win][C] -> [B][Hout][Wout][C], F.interpolate(mode="nearest")'s indices (C's bytes % 16 == 0)"""
    _require_cuda(x)
    B, Hin, Win, Cc = x.shape
    out = _out(out, (B, Hout, Wout, Cc), x.dtype, x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().dsim_op_resize_nearest(x.data_ptr(), out.data_ptr(), B, Hin, Win, int(Hout), int(Wout), Cc * x.element_size(),
                                                     _stream_ptr()), "op_resize_nearest")
    return out.view(B, Hout, Wout, Cc)


def op_gather_ctx(ctx, index, dtype, out=None):
    """ctx f32 [n_ctx][2][per...], index int32 [n_images] -> [2 n_images][per...] in dtype; row (2 i + cfg) = ctx[clamp(index[i])][cfg]"""
    _require_cuda(ctx, index)
    _f32((ctx, "ctx"))
    if index.dtype != torch.int32 or ctx.ndim < 3 or ctx.shape[1] != 2:
        raise _lib.DsimError("gather_ctx: ctx f32 [n_ctx][2][...], index int32 [n_images]")
    n_ctx, n = ctx.shape[0], index.numel()
    per = ctx[0, 0].numel()
    shape = (2 * n,) + tuple(ctx.shape[2:])
    out = _out(out, shape, dtype, ctx.device)
    with torch.cuda.device(ctx.device):
        _lib.check(_lib.lib().dsim_op_gather_ctx(ctx.data_ptr(), n_ctx, index.data_ptr(), out.data_ptr(), _TORCH2DSIM[dtype], n, per,
                                                 _stream_ptr()), "op_gather_ctx")
    return out.view(shape)


def op_patch_embed(lat, noise, sa, sb, w, bias, pos, p, dtype, out=None):
    """DiT's patch embedding of the noised latent: lat / noise f32 [n][Cin][S][S], w f32 [D][Cin][p][p], bias f32 [D], pos f32 [T][D]
    -> [2 n][T][D] in dtype (both CFG halves), T = (S / p)^2"""
    _require_cuda(lat, noise, w, bias, pos)
    _f32((lat, "lat"), (noise, "noise"), (w, "w"), (bias, "bias"), (pos, "pos"))
    n, Cin, S, S2 = lat.shape
    D = w.shape[0]
    T = (S // p) ** 2
    if S != S2 or noise.shape != lat.shape or w.numel() != D * Cin * p * p or bias.numel() != D or pos.numel() != T * D:
        raise _lib.DsimError("patch_embed: lat / noise [n][Cin][S][S], w [D][Cin][p][p], bias [D], pos [T][D]")
    out = _out(out, (2 * n, T, D), dtype, lat.device)
    with torch.cuda.device(lat.device):
        _lib.check(_lib.lib().dsim_op_patch_embed(lat.data_ptr(), noise.data_ptr(), float(sa), float(sb), w.data_ptr(), bias.data_ptr(),
                                                  pos.data_ptr(), out.data_ptr(), _TORCH2DSIM[dtype], n, Cin, S, int(p), D, _stream_ptr()),
                   "op_patch_embed")
    return out.view(2 * n, T, D)


def op_fold_quant(wq, wco=None, bco=None, bq=None, out_w=None, out_b=None):
    """The VAE's quant_conv folded into conv_out: wq f32 [Cm][Cm]; with wco [Cm][K] (compute dtype) the weight wq wco in that dtype,
    with bco / bq f32 [Cm] the bias wq bco + bq in f32 -> (weight or None, bias or None)."""
    _require_cuda(wq, wco, bco, bq)
    _f32((wq, "wq"), (bco, "bco"), (bq, "bq"))
    Cm = wq.shape[0]
    if tuple(wq.shape) != (Cm, Cm) or (wco is not None and wco.shape[0] != Cm) or any(t is not None and t.numel() != Cm for t in (bco, bq)):
        raise _lib.DsimError("fold_quant: wq [Cm][Cm], wco [Cm][K], bco / bq [Cm]")
    K = wco.shape[1] if wco is not None else 1
    dt = wco.dtype if wco is not None else torch.float32
    ow = _out(out_w, (Cm, K), dt, wq.device) if wco is not None else None
    ob = _out(out_b, (Cm,), torch.float32, wq.device) if bco is not None else None
    with torch.cuda.device(wq.device):
        _lib.check(_lib.lib().dsim_op_fold_quant(wq.data_ptr(), _ptr(wco), _ptr(bco), _ptr(bq), _ptr(ow), _ptr(ob), Cm, K, _TORCH2DSIM[dt],
                                                 _stream_ptr()), "op_fold_quant")
    return ow, ob


def op_to_nchw_f32(x, out=None):
    """token-major [n][HW][C] in any of the three dtypes -> f32 [n][C][HW]"""
    _require_cuda(x)
    n, HW, Cc = x.shape
    out = _out(out, (n, Cc, HW), torch.float32, x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().dsim_op_to_nchw_f32(x.data_ptr(), out.data_ptr(), n, HW, Cc, _TORCH2DSIM[x.dtype], _stream_ptr()),
                   "op_to_nchw_f32")
    return out.view(n, Cc, HW)


def groupnorm_plan(C0, C1, B, HW, groups, dtype, pre=False):
    """What op_groupnorm (op_groupnorm_pre with pre) launches for this shape: dict(form "onepass" / "twopass" / "pre", NS, UNR, CS,
    tpr, R, chunks, rb), from the function the launcher itself calls.  Host only; raises DsimError where the launch would refuse."""
    p = _lib.GnPlanC()
    _lib.check(_lib.lib().dsim_groupnorm_plan(int(C0), int(C1), int(B), int(HW), int(groups), _TORCH2DSIM[dtype], int(bool(pre)),
                                              C.byref(p)), "groupnorm_plan")
    d = {n: getattr(p, n) for n, _ in p._fields_}
    d["form"] = _lib.GN_FORMS[p.form]
    return d


def layernorm_plan(M, Cc, dtype, mod=False):
    """What op_layernorm (op_layernorm_mod with mod) launches: dict(form "rows" / "wave", LPR, CPL, passes, MAXS, RPW, blocks)."""
    p = _lib.LnPlanC()
    _lib.check(_lib.lib().dsim_layernorm_plan(int(M), int(Cc), _TORCH2DSIM[dtype], int(bool(mod)), C.byref(p)), "layernorm_plan")
    d = {n: getattr(p, n) for n, _ in p._fields_}
    d["form"] = _lib.LN_FORMS[p.form]
    return d


def op_attention(q, k, v, heads, fp8: bool = False):
    """q: [B][Nq][H*D]; k,v: [Bkv][Nk][H*D] -> [B][Nq][H*D].  fp8: bf16 tensors, e4m3 MFMAs (DiT config 5)."""
    L = _lib.lib()
    _require_cuda(q, k, v)
    B, Nq, HD = q.shape
    Bkv, Nk, _ = k.shape
    out = torch.empty_like(q)
    if fp8:
        if q.dtype != torch.bfloat16:
            raise _lib.DsimError("fp8 attention takes bf16 tensors")
        _lib.check(L.dsim_op_attention_fp8(q.data_ptr(), HD, k.data_ptr(), v.data_ptr(), HD, out.data_ptr(), HD, B, Bkv, heads,
                                           Nq, Nk, HD // heads, _stream_ptr()), "op_attention_fp8")
        return out
    _lib.check(L.dsim_op_attention(q.data_ptr(), HD, k.data_ptr(), v.data_ptr(), HD, out.data_ptr(), HD, B, Bkv, heads,
                                   Nq, Nk, HD // heads, _TORCH2DSIM[q.dtype], _stream_ptr()), "op_attention")
    return out


_PLAN_ADDR = 1 << 12     # attention_plan's default operand address: 256-byte aligned, never dereferenced


def attention_plan(B, Bkv, heads, Nq, Nk, D, dtype, *, ldq=None, ldk=None, ldo=None, q=_PLAN_ADDR, k=_PLAN_ADDR, v=_PLAN_ADDR,
                   out=_PLAN_ADDR, fp8=False):
    """The kernel dsim_op_attention_ex would launch for these arguments, by its _lib.ATTN_KINDS name; host only (launches nothing, reads
    no memory: q / k / v / out are addresses, looked at for their alignment only).  ld's default to heads * D; raises DsimError where
    the launch would refuse the arguments."""
    L = _lib.lib()
    HD = heads * D
    kind = C.c_int(-1)
    _lib.check(L.dsim_attention_plan(int(q) or None, int(ldq or HD), int(k) or None, int(v) or None, int(ldk or HD), int(out) or None,
                                     int(ldo or HD), B, Bkv, heads, Nq, Nk, D, _TORCH2DSIM[dtype], int(bool(fp8)), C.byref(kind)),
               "attention_plan")
    return _lib.ATTN_KINDS[kind.value]


def op_attention_rows(q, q_off, ldq, k, k_off, v, v_off, ldk, out, o_off, ldo, *, B, Bkv, heads, Nq, Nk, D, fp8=False):
    """The attention on the executors' fused-row buffers (dsim_op_attention_ex): head h of query row (b, i) is q[(b Nq + i) ldq + q_off
    + h D ...], of key row (b', j) k[(b' Nk + j) ldk + k_off + h D ...] and v[... + v_off ...], of output row (b, i) out[(b Nq + i) ldo
    + o_off + h D ...]; offsets and ld's count elements of the flat (contiguous) tensors, which may be the same tensor (self-attention's
    q | k | v rows: ldq = ldk = 3C, k_off = C, v_off = 2C).  fp8: bf16 tensors, e4m3 MFMAs.  Writes out in place and returns the launch
    record: kind (an _lib.ATTN_KINDS name), D, dtype, k80, qit, grid and family (the executors' profile family name)."""
    L = _lib.lib()
    _require_cuda(q, k, v, out)
    dt = q.dtype
    if dt not in _TORCH2DSIM or any(t.dtype != dt for t in (k, v, out)):
        raise _lib.DsimError("q, k, v and out must share one float32 / bfloat16 / float16 dtype")
    HD = heads * D
    for t, off, ld, rows, nm in ((q, q_off, ldq, B * Nq, "q"), (k, k_off, ldk, Bkv * Nk, "k"), (v, v_off, ldk, Bkv * Nk, "v"),
                                 (out, o_off, ldo, B * Nq, "out")):
        if off < 0 or off + HD > ld or (rows - 1) * ld + off + HD > t.numel():
            raise _lib.DsimError(f"{nm}: {rows} rows of {ld} elements from offset {off} do not fit its {t.numel()} elements")
    es = q.element_size()
    rec = _lib.AttnLaunchC()
    with torch.cuda.device(q.device):
        _lib.check(L.dsim_op_attention_ex(q.data_ptr() + q_off * es, int(ldq), k.data_ptr() + k_off * es, v.data_ptr() + v_off * es,
                                          int(ldk), out.data_ptr() + o_off * es, int(ldo), B, Bkv, heads, Nq, Nk, D, _TORCH2DSIM[dt],
                                          int(bool(fp8)), C.byref(rec), _stream_ptr()), "op_attention_rows")
    return {"kind": _lib.ATTN_KINDS[rec.kind], "D": rec.D, "dtype": {0: torch.float32, 1: torch.bfloat16, 2: torch.float16}[rec.dtype],
            "k80": bool(rec.k80), "qit": rec.qit, "grid": rec.grid, "family": rec.family.decode()}


def op_softmax_rows(x, scale):
    """softmax(x * scale) along the last dim of a contiguous [rows][cols] tensor (the VAE mid-block's softmax_rows_kernel)"""
    L = _lib.lib()
    _require_cuda(x)
    out = torch.empty_like(x)
    rows, cols = x.shape
    _lib.check(L.dsim_op_softmax_rows(x.data_ptr(), out.data_ptr(), rows, cols, float(scale), _TORCH2DSIM[x.dtype], _stream_ptr()),
               "op_softmax_rows")
    return out


# ---- the arithmetic either side of the VAE encoder, on the device ------------------------------------------------
def image_preprocess(pixels_u8: torch.Tensor, to_half: bool = False) -> torch.Tensor:
    """pixels u8 cuda [n][H][W][3] (decoded + Lanczos-resized on the host) -> process_image's f32 [n][3][H][W], bit-identical
    to the numpy arithmetic of /root/reference/diffsim/diffsim.py:31-41; to_half rounds through fp16 (diffsim.py:93)."""
    L = _lib.lib()
    _require_cuda(pixels_u8)
    if pixels_u8.dtype != torch.uint8 or pixels_u8.ndim != 4 or pixels_u8.shape[3] != 3:
        raise _lib.DsimError("pixels must be uint8 [n][H][W][3]")
    n, H, W, _ = pixels_u8.shape
    out = torch.empty((n, 3, H, W), dtype=torch.float32, device=pixels_u8.device)
    _lib.check(L.dsim_image_preprocess(pixels_u8.contiguous().data_ptr(), out.data_ptr(), n, H, W, int(to_half), _stream_ptr()),
               "dsim_image_preprocess")
    return out


def latent_sample(moments: torch.Tensor, eps: torch.Tensor, scaling_factor: float, first: int = 0, stride: int = 1,
                  round_fp16: bool = False) -> torch.Tensor:
    """scaling_factor * DiagonalGaussianDistribution(moments).sample() with the caller's draw `eps` ((1,C,h,w) shared or
    (n_out,C,h,w)), for images first, first+stride, ... of `moments` ((n,2C,h,w) f32 cuda) -> (n_out,C,h,w) f32."""
    L = _lib.lib()
    moments, eps = moments.contiguous(), eps.contiguous()
    _require_cuda(moments, eps)
    n, C2, h, w = moments.shape
    Cc = C2 // 2
    n_out = (n - first + stride - 1) // stride
    if moments.dtype != torch.float32 or eps.dtype != torch.float32 or eps.shape[1:] != (Cc, h, w) or eps.shape[0] not in (1, n_out):
        raise _lib.DsimError("latent_sample: moments (n,2C,h,w) f32, eps (1|n_out,C,h,w) f32")
    out = torch.empty((n_out, Cc, h, w), dtype=torch.float32, device=moments.device)
    _lib.check(L.dsim_latent_sample(moments.data_ptr(), eps.data_ptr(), out.data_ptr(), n_out, first,
                                    stride, Cc, h * w, eps.shape[0], float(scaling_factor), int(round_fp16), _stream_ptr()),
               "dsim_latent_sample")
    return out


# ---- PIL's resize on the device (csrc/resize.hip; tables and served range: resize.py) -----------------------------
RESIZE_CHUNK_BYTES = 256 << 20                  # source bytes per upload, at most (a larger single image goes alone)
RESIZE_COUNTS = {"gpu": 0, "fallback": 0}       # images resize_u8 resized on the device / on the host since the process started
_resize_staging: Dict[str, tuple] = {}          # device -> (pinned uint8 buffer, the event after its last upload)
_resize_lock = threading.Lock()                 # one resize_u8 at a time fills the staging buffer and moves the counts


def _resize_stage(dev: torch.device, nbytes: int) -> torch.Tensor:
    """The pinned upload buffer of `dev`, grown to nbytes, free to overwrite (the upload that last read it has finished)."""
    buf, ev = _resize_staging.get(str(dev), (None, None))
    if ev is not None:
        ev.synchronize()
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, pin_memory=True)
    _resize_staging[str(dev)] = (buf, None)
    return buf


def resize_u8(sources, out_w: int, out_h: int, filter: str, crop=None, device=None) -> torch.Tensor:
    """``Image.resize((out_w, out_h), filter)`` then ``.crop`` to crop = (ox, oy, cw, ch) (None: everything) of every source: a list
    of uint8 (h, w, 3) host arrays or tensors of any sizes -> uint8 cuda (n, ch, cw, 3), PIL's bytes.  filter: "lanczos" or
    "bicubic".  The sources go up packed, one upload per chunk of RESIZE_CHUNK_BYTES, with the coefficient tables of the chunk
    (resize.coeff_table, one per distinct extent) in front; dsim_resize_u8 does the rest.  A source outside resize.served is
    resized by PIL on the host and copied into its slot.  RESIZE_COUNTS counts both kinds.  Calls from several threads take turns
    (one pinned staging buffer per device)."""
    import numpy as np
    from . import resize as rz
    L = _lib.lib()
    if filter not in rz.FILTERS:
        raise _lib.DsimError(f"resize_u8: filter {filter!r} (lanczos or bicubic)")
    out_w, out_h = int(out_w), int(out_h)
    ox, oy, cw, ch = (0, 0, out_w, out_h) if crop is None else (int(v) for v in crop)
    if out_w < 1 or out_h < 1 or cw < 1 or ch < 1 or ox < 0 or oy < 0 or ox + cw > out_w or oy + ch > out_h:
        raise _lib.DsimError(f"resize_u8: crop {(ox, oy, cw, ch)} outside the {out_w}x{out_h} output")
    arrays = []
    for s in sources:
        a = s.numpy() if isinstance(s, torch.Tensor) else np.asarray(s)
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
            raise _lib.DsimError("resize_u8: every source is a uint8 (h, w, 3) host array")
        arrays.append(a)
    if not arrays:
        raise _lib.DsimError("resize_u8: no sources")
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    out = torch.empty((len(arrays), ch, cw, 3), dtype=torch.uint8, device=dev)
    tstride = (cw * 3 + 15) // 16 * 16
    chunk, chunk_bytes, first = [], 0, 0          # consecutive served sources, their bytes, the first one's slot

    def flush():
        nonlocal chunk, chunk_bytes
        if not chunk:
            return
        tables, table_arrays, t_ints = {}, [], 0

        def table(n_in, n_out):
            nonlocal t_ints
            if n_in == n_out:
                return -1, None
            key = (n_in, n_out)
            if key not in tables:
                b, k = rz.coeff_table(n_in, n_out, filter)
                tables[key] = (len(tables), t_ints, k.shape[1], b)
                table_arrays.extend((b, k))
                t_ints += b.size + k.size
            return tables[key][0], tables[key][3]
        imgs = (_lib.ResizeImageC * len(chunk))()
        ids = [table(a.shape[1], out_w) + table(a.shape[0], out_h) for a in chunk]
        if not tables:                                  # every pass skipped: one table nobody reads, so that the count is >= 1
            tables[(1, 1)] = (0, 0, 1, None)
            table_arrays, t_ints = [np.zeros(4, np.int32)], 4
        t_bytes = (t_ints * 4 + 15) // 16 * 16
        temp = src_bytes = 0
        for d, a, (ht, _, vt, vb) in zip(imgs, chunk, ids):
            h, w, _ = a.shape
            y0, rows = oy, ch
            if vb is not None:
                y0 = int(vb[oy, 0])
                rows = int(vb[oy + ch - 1, 0] + vb[oy + ch - 1, 1]) - y0
            d.src_offset, d.w, d.h, d.h_table, d.v_table, d.y_first, d.rows, d.temp_offset = src_bytes, w, h, ht, vt, y0, rows, temp
            if ht >= 0:
                temp += rows * tstride
            src_bytes += (a.size + 15) // 16 * 16
        tabs = (_lib.ResizeTableC * len(tables))()
        for (n_in, n_out), (i, o, ksize, _) in tables.items():
            tabs[i].offset, tabs[i].in_size, tabs[i].out_size, tabs[i].ksize = o, n_in, n_out, ksize
        total = t_bytes + src_bytes
        stage = _resize_stage(dev, total)
        host = stage.numpy()
        p = 0
        for t in table_arrays:
            host[p:p + t.size * 4] = np.ascontiguousarray(t).view(np.uint8).reshape(-1)
            p += t.size * 4
        for d, a in zip(imgs, chunk):
            host[t_bytes + d.src_offset:t_bytes + d.src_offset + a.size] = a.reshape(-1)
        up = torch.empty(total, dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            up.copy_(stage[:total], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            _resize_staging[str(dev)] = (stage, ev)
            args = (imgs, len(chunk), tabs, len(tables), t_ints, out_w, out_h, ox, oy, cw, ch, src_bytes)
            ws_bytes = L.dsim_resize_u8_workspace_bytes(*args)
            if ws_bytes == 0:
                raise _lib.DsimError("dsim_resize_u8 refuses this call (include/diffsim_amd.h lists the refusals)")
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            dst = out[first:first + len(chunk)]
            _lib.check(L.dsim_resize_u8(up.data_ptr() + t_bytes, src_bytes, imgs, len(chunk), up.data_ptr(), t_ints, tabs, len(tables),
                                        out_w, out_h, ox, oy, cw, ch, dst.data_ptr(), ws.data_ptr(), ws_bytes, _stream_ptr()),
                       "dsim_resize_u8")
        RESIZE_COUNTS["gpu"] += len(chunk)
        chunk, chunk_bytes = [], 0

    with _resize_lock:
        for i, a in enumerate(arrays):
            h, w, _ = a.shape
            if not rz.served(w, h, out_w, out_h):
                from PIL import Image
                im = Image.fromarray(np.ascontiguousarray(a)).resize((out_w, out_h), resample=getattr(Image.Resampling, filter.upper()))
                out[i] = torch.from_numpy(np.asarray(im.crop((ox, oy, ox + cw, oy + ch))).copy()).to(dev)
                RESIZE_COUNTS["fallback"] += 1
                flush()
                continue
            if chunk and (chunk_bytes + a.size > RESIZE_CHUNK_BYTES or len(chunk) >= 32768):
                flush()
            if not chunk:
                first = i
            chunk.append(a)
            chunk_bytes += a.size
        flush()
    return out


# ---- VAE encoder ------------------------------------------------------------
class _LatentDist:
    """``DiagonalGaussianDistribution`` surface the reference uses: ``.sample(generator)``
    (diffsim/diffsim.py:94).  The moments live on the device; the noise is drawn with the caller's
    generator on ITS device (CPU in the reference-CPU-path setting) in the reference's order, and
    mean + exp(0.5 clamp(logvar)) * eps is one launch of dsim_latent_sample -- the same arithmetic the batched paths use,
    so a per-pair call and a chunked run give bit-identical latents."""

    def __init__(self, moments: torch.Tensor, sample_dtype: torch.dtype = torch.float32):
        self.moments = moments
        # dtype of the sample draw: diffusers draws randn_tensor(dtype=parameters.dtype), i.e. fp16 under the
        # reference's fp16 SD1.5 pipeline -- a different random stream from the fp32 draw of the same generator
        self.sample_dtype = sample_dtype

    @property
    def mean(self) -> torch.Tensor:
        return self.moments.chunk(2, dim=1)[0]

    @property
    def logvar(self) -> torch.Tensor:
        return self.moments.chunk(2, dim=1)[1].clamp(-30.0, 20.0)

    @property
    def std(self) -> torch.Tensor:
        return torch.exp(0.5 * self.logvar)

    def sample(self, generator=None) -> torch.Tensor:
        gdev = generator.device if generator is not None else self.moments.device
        eps = torch.randn(self.mean.shape, generator=generator, dtype=self.sample_dtype, device=gdev)
        return latent_sample(self.moments.float(), eps.to(self.moments.device, torch.float32), 1.0)

    def mode(self) -> torch.Tensor:
        return self.mean


class _EncodeOut:
    def __init__(self, moments, sample_dtype=torch.float32):
        self.latent_dist = _LatentDist(moments, sample_dtype)


class VAEEncoder(_Handle):
    """``AutoencoderKL.encode`` on the HIP engine, with the surface DiffSim.prepare_image_latents needs:
    ``vae.encode(image).latent_dist.sample(generator)`` and ``vae.config.scaling_factor``."""

    prefix = "vae"

    def __init__(self, cfg, state_dict: Dict[str, torch.Tensor], dtype: torch.dtype = torch.bfloat16,
                 device: str = "cuda:0"):
        import types
        self.L = _lib.lib()
        if not torch.cuda.is_available():
            raise _lib.DsimError("no GPU visible: the VAE encoder runs only on the HIP device")
        self.cfg, self.dtype, self.device = cfg, dtype, torch.device(device)
        self.config = types.SimpleNamespace(scaling_factor=cfg.scaling_factor)
        c = _lib.VAECfgC()
        c.in_channels, c.latent_channels, c.n_levels = cfg.in_channels, cfg.latent_channels, len(cfg.block_out_channels)
        for i, v in enumerate(cfg.block_out_channels):
            c.block_out_channels[i] = v
        c.layers_per_block, c.norm_num_groups = cfg.layers_per_block, cfg.norm_num_groups
        c.compute_dtype = _TORCH2DSIM[dtype]
        self._create_and_load(c, state_dict, lambda k: k.startswith("encoder.") or k.startswith("quant_conv."))
        self.sample_dtype = torch.float32      # dtype of latent_dist.sample's draw (DiffSim(noise_dtype=...) sets it)

    def moments(self, images: torch.Tensor) -> torch.Tensor:
        """images (n,3,S,S) in [-1,1], any float dtype/device -> moments (n, 2*latent, S/8, S/8) f32 on device."""
        x = images.to(self.device).float().contiguous()      # an fp16 image keeps its fp16-rounded pixel values
        n, cin, S, S2 = x.shape
        if cin != self.cfg.in_channels or S != S2:
            raise _lib.DsimError("images must be (n, in_channels, S, S)")
        f = 2 ** (len(self.cfg.block_out_channels) - 1)
        out = torch.empty((n, 2 * self.cfg.latent_channels, S // f, S // f), dtype=torch.float32, device=self.device)
        # the kernels address activations through 32-bit buffer offsets: keep every tensor < 2 GiB
        es = 4 if self.dtype == torch.float32 else 2
        chunk = max(1, (2 ** 30) // (S * S * max(self.cfg.block_out_channels[0], 1) * es))
        with torch.cuda.device(self.device):
            for i0 in range(0, n, chunk):
                m = min(chunk, n - i0)
                need = int(self.L.dsim_vae_workspace_bytes(self._h, m, S))
                if need == 0:
                    raise _lib.DsimError("unsupported image size for the VAE encoder")
                ws = self._arena(need)
                _lib.check(self.L.dsim_vae_encode(self._h, x[i0:i0 + m].data_ptr(), m, S, out[i0:i0 + m].data_ptr(),
                                                  ws.data_ptr(), ws.numel(), _stream_ptr()), "dsim_vae_encode")
        return out

    def encode(self, images: torch.Tensor) -> _EncodeOut:
        return _EncodeOut(self.moments(images), self.sample_dtype)


# ---- DiT backbone ---------------------------------------------------------
class DiTEngine(_Handle):
    """One handle = (DiT config, compute dtype, tapped block)."""

    prefix = "dit"

    def __init__(self, cfg, state_dict: Dict[str, torch.Tensor], dtype: torch.dtype = torch.bfloat16, target_layer: int = 0,
                 device: str = "cuda:0"):
        self.L = _lib.lib()
        if not torch.cuda.is_available():
            raise _lib.DsimError("no GPU visible: the DiT engine runs only on the HIP device")
        self.cfg, self.dtype, self.device = cfg, dtype, torch.device(device)
        c = _lib.DiTCfgC()
        for f in ("input_size", "patch_size", "in_channels", "hidden_size", "depth", "num_heads", "mlp_ratio", "num_classes",
                  "freq_dim"):
            setattr(c, f, getattr(cfg, f))
        c.compute_dtype, c.tap_layer = _TORCH2DSIM[dtype], int(target_layer)
        self.target_layer = int(target_layer)
        self.tokens = (cfg.input_size // cfg.patch_size) ** 2
        self.heads, self.head_dim = cfg.num_heads, cfg.hidden_size // cfg.num_heads
        self._create_and_load(c, state_dict, lambda k: not k.startswith("final_layer"))
        self._cond = None

    def set_tap(self, layer: int):
        """Move the tapped block; the packed weights are shared by every --target_layer (dsim_dit_set_tap)."""
        if int(layer) != self.target_layer:
            _lib.check(self.L.dsim_dit_set_tap(self._h, int(layer)), "dsim_dit_set_tap")
            self.target_layer = int(layer)

    def set_attention(self, fp8: bool):
        """fp8 (OCP e4m3) MFMA attention in the DiT blocks (BASELINE config 5); bf16 handles only."""
        _lib.check(self.L.dsim_dit_set_attention(self._h, 1 if fp8 else 0), "dsim_dit_set_attention")

    def set_conditioning(self, t_model: int, y0: int, y1: int):
        if self._cond != (t_model, y0, y1):
            with torch.cuda.device(self.device):
                _lib.check(self.L.dsim_dit_set_conditioning(self._h, int(t_model), int(y0), int(y1), _stream_ptr()),
                           "dit set_conditioning")
            self._cond = (t_model, y0, y1)

    def qkv(self, latents: torch.Tensor, noise: torch.Tensor, sa: float, sb: float):
        _require_cuda(latents, noise)
        n = latents.shape[0]
        s = self.cfg.input_size
        if tuple(latents.shape) != (n, self.cfg.in_channels, s, s) or latents.dtype != torch.float32 or noise.shape != latents.shape:
            raise _lib.DsimError(f"latents/noise must be float32 (n,{self.cfg.in_channels},{s},{s})")
        with torch.cuda.device(self.device):
            need = int(self.L.dsim_dit_workspace_bytes(self._h, n))
            ws = self._arena(need)
            shape = (n, 2, self.tokens, self.cfg.hidden_size)
            q, k, v = (torch.empty(shape, dtype=self.dtype, device=self.device) for _ in range(3))
            _lib.check(self.L.dsim_dit_qkv(self._h, latents.data_ptr(), noise.data_ptr(), float(sa), float(sb), n, q.data_ptr(),
                                           k.data_ptr(), v.data_ptr(), ws.data_ptr(), ws.numel(), _stream_ptr()),
                       "dsim_dit_qkv")
        return q, k, v

    # ---- tap sweeps: the q,k,v of several blocks from one forward (dsim_dit_qkv_taps) ----------------------------------
    def taps_workspace_bytes(self, n_images: int, layers) -> int:
        """Workspace of one qkv_taps call over n_images (0: the call is impossible -- see dsim_dit_taps_workspace_bytes)."""
        arr = (C.c_int * max(1, len(layers)))(*[int(l) for l in layers])
        return int(self.L.dsim_dit_taps_workspace_bytes(self._h, n_images, len(layers), arr))

    def max_images_taps(self, layers, upper: int = 4096) -> int:
        """Largest n_images one qkv_taps call accepts (every activation and tap output < 2 GiB)."""
        return self._largest(lambda m: self.taps_workspace_bytes(m, layers) > 0, upper)

    def qkv_taps(self, latents: torch.Tensor, noise: torch.Tensor, sa: float, sb: float, layers):
        """qkv() at every block of `layers` (any order, no repeats) from ONE forward to the deepest: entry i is bit for bit what
        qkv() returns with the tap at layers[i].  The handle's own tap does not move."""
        _require_cuda(latents, noise)
        n, nt = latents.shape[0], len(layers)
        s = self.cfg.input_size
        if tuple(latents.shape) != (n, self.cfg.in_channels, s, s) or latents.dtype != torch.float32 or noise.shape != latents.shape:
            raise _lib.DsimError(f"latents/noise must be float32 (n,{self.cfg.in_channels},{s},{s})")
        if nt < 1:
            raise _lib.DsimError("qkv_taps: no taps")
        try:
            arr = (C.c_int * nt)(*[int(l) for l in layers])
        except (TypeError, ValueError):
            raise _lib.DsimError(f"unknown taps {layers!r}") from None
        with torch.cuda.device(self.device):
            need = self.taps_workspace_bytes(n, layers)
            ws = self._arena(need) if need else torch.empty(256, dtype=torch.uint8, device=self.device)
            shape = (n, 2, self.tokens, self.cfg.hidden_size) if need else (1,)
            outs = [tuple(torch.empty(shape, dtype=self.dtype, device=self.device) for _ in range(3)) for _ in range(nt)]
            ptr = lambda j: (C.c_void_p * nt)(*[o[j].data_ptr() for o in outs])
            st = self.L.dsim_dit_qkv_taps(self._h, latents.data_ptr(), noise.data_ptr(), float(sa), float(sb), n, nt, arr, ptr(0),
                                          ptr(1), ptr(2), ws.data_ptr(), ws.numel() if need else 0, _stream_ptr())
            if not need and st in (0, -3):
                raise _lib.DsimError(f"{n} images do not fit one sweep call (an activation or a tap output would reach 2 GiB)")
            _lib.check(st, "dsim_dit_qkv_taps")
        return outs


# ---- ViT backbones: the reference's clip_cross / dino_cross metrics ----------------------------------------------------
def interpolate_pos_embed(pos: torch.Tensor, grid: int) -> torch.Tensor:
    """A stored position table (1 + g0^2, C) at a grid x grid patch grid: the class row kept, the patch rows bicubically
    interpolated in f32 (align_corners False) as HF Dinov2Embeddings.interpolate_pos_encoding does; unchanged when g0 == grid."""
    g0 = int(round((pos.shape[0] - 1) ** 0.5))
    if g0 * g0 != pos.shape[0] - 1:
        raise _lib.DsimError(f"position table of {pos.shape[0]} rows: not 1 + a square grid")
    if g0 == grid:
        return pos
    patch = pos[1:].float().reshape(1, g0, g0, -1).permute(0, 3, 1, 2)
    patch = torch.nn.functional.interpolate(patch, size=(grid, grid), mode="bicubic", align_corners=False)
    return torch.cat([pos[:1].float(), patch.permute(0, 2, 3, 1).reshape(grid * grid, -1)]).contiguous()


class ViTEngine(_Handle):
    """One handle = (ViT config, compute dtype, image side, tapped layer).  state_dict: the neutral keys of config.vit_param_shapes,
    the position table at its stored grid (interpolated here, on the host, to the side's grid -- DINOv2 only: CLIP has one side)."""

    prefix = "vit"

    def __init__(self, cfg, state_dict: Dict[str, torch.Tensor], dtype: torch.dtype = torch.bfloat16, target_layer: int = 0,
                 device: str = "cuda:0", side: Optional[int] = None):
        self.L = _lib.lib()
        if not torch.cuda.is_available():
            raise _lib.DsimError("no GPU visible: the ViT engine runs only on the HIP device")
        side = cfg.image_size if side is None else int(side)
        if side % cfg.patch_size or side < cfg.patch_size:
            raise _lib.DsimError(f"image side {side} is not a multiple of the patch size {cfg.patch_size}")
        grid = side // cfg.patch_size
        if cfg.kind == "clip" and grid != cfg.pos_grid:
            raise _lib.DsimError(f"CLIP position table serves {cfg.pos_grid * cfg.patch_size} px only (no interpolation): got {side}")
        self.cfg, self.dtype, self.device, self.side = cfg, dtype, torch.device(device), side
        c = _lib.ViTCfgC()
        c.image_size = side
        for f in ("patch_size", "hidden_size", "depth", "num_heads", "mlp_dim"):
            setattr(c, f, getattr(cfg, f))
        c.act, c.tap_input = _lib.VIT_ACT[cfg.act], _lib.VIT_TAP_INPUT[cfg.tap_input]
        c.pre_norm, c.patch_bias, c.layer_scale = int(cfg.pre_norm), int(cfg.patch_bias), int(cfg.layer_scale)
        c.ln_eps, c.compute_dtype, c.tap_layer = float(cfg.ln_eps), _TORCH2DSIM[dtype], int(target_layer)
        self.target_layer = int(target_layer)
        self.tokens = cfg.tokens(side)
        self.heads, self.head_dim = cfg.num_heads, cfg.hidden_size // cfg.num_heads
        sd = dict(state_dict)
        sd["pos_embed"] = interpolate_pos_embed(sd["pos_embed"], grid)
        self._create_and_load(c, sd)

    def set_tap(self, layer: int):
        """Move the tapped layer; the packed weights are shared by every --target_layer (dsim_vit_set_tap)."""
        if int(layer) != self.target_layer:
            _lib.check(self.L.dsim_vit_set_tap(self._h, int(layer)), "dsim_vit_set_tap")
            self.target_layer = int(layer)

    def _check_pixels(self, pixels: torch.Tensor) -> int:
        _require_cuda(pixels)
        n = pixels.shape[0]
        if tuple(pixels.shape) != (n, 3, self.side, self.side) or pixels.dtype != torch.float32 or n < 1:
            raise _lib.DsimError(f"pixels must be float32 (n,3,{self.side},{self.side}): {tuple(pixels.shape)} {pixels.dtype}")
        return n

    def workspace_bytes(self, n_images: int) -> int:
        return int(self.L.dsim_vit_workspace_bytes(self._h, n_images))

    def max_images(self, upper: int = 4096) -> int:
        """Largest n_images one qkv call accepts (every activation < 2 GiB)."""
        return self._largest(lambda m: self.workspace_bytes(m) > 0, upper)

    def qkv(self, pixels: torch.Tensor):
        """pixels: normalised f32 (n, 3, S, S) on the device -> q, k, v (n, 1, N, C) in the compute dtype, the class token first."""
        n = self._check_pixels(pixels)
        with torch.cuda.device(self.device):
            need = self.workspace_bytes(n)
            if not need:
                raise _lib.DsimError(f"{n} images do not fit one call (an activation would reach 2 GiB)")
            ws = self._arena(need)
            shape = (n, 1, self.tokens, self.cfg.hidden_size)
            q, k, v = (torch.empty(shape, dtype=self.dtype, device=self.device) for _ in range(3))
            _lib.check(self.L.dsim_vit_qkv(self._h, pixels.data_ptr(), n, q.data_ptr(), k.data_ptr(), v.data_ptr(), ws.data_ptr(),
                                           ws.numel(), _stream_ptr()), "dsim_vit_qkv")
        return q, k, v

    # ---- tap sweeps: the q,k,v of several layers from one forward (dsim_vit_qkv_taps) ---------------------------------------
    def taps_workspace_bytes(self, n_images: int, layers) -> int:
        arr = (C.c_int * max(1, len(layers)))(*[int(l) for l in layers])
        return int(self.L.dsim_vit_taps_workspace_bytes(self._h, n_images, len(layers), arr))

    def max_images_taps(self, layers, upper: int = 4096) -> int:
        return self._largest(lambda m: self.taps_workspace_bytes(m, layers) > 0, upper)

    def qkv_taps(self, pixels: torch.Tensor, layers):
        """qkv() at every layer of `layers` (any order, no repeats) from ONE forward to the deepest: entry i is bit for bit what
        qkv() returns with the tap at layers[i].  The handle's own tap does not move."""
        n, nt = self._check_pixels(pixels), len(layers)
        if nt < 1:
            raise _lib.DsimError("qkv_taps: no taps")
        try:
            arr = (C.c_int * nt)(*[int(l) for l in layers])
        except (TypeError, ValueError):
            raise _lib.DsimError(f"unknown taps {layers!r}") from None
        with torch.cuda.device(self.device):
            need = self.taps_workspace_bytes(n, layers)
            if not need:
                raise _lib.DsimError(f"taps {list(layers)!r} of {n} images: an invalid or repeated layer, or an activation would reach 2 GiB")
            ws = self._arena(need)
            shape = (n, 1, self.tokens, self.cfg.hidden_size)
            outs = [tuple(torch.empty(shape, dtype=self.dtype, device=self.device) for _ in range(3)) for _ in range(nt)]
            ptr = lambda j: (C.c_void_p * nt)(*[o[j].data_ptr() for o in outs])
            _lib.check(self.L.dsim_vit_qkv_taps(self._h, pixels.data_ptr(), n, nt, arr, ptr(0), ptr(1), ptr(2), ws.data_ptr(), ws.numel(),
                                                _stream_ptr()), "dsim_vit_qkv_taps")
        return outs


# ---- VGG Gram style metric: the conv stack and the Gram rows (csrc/vgg.hip) ---------------------------------------------------
class VGGEngine(_Handle):
    """One handle = (plan, compute dtype).  plan: conv output channels and "P" / 0 for the 2x2 max-pools, e.g. config.VGG19_PLAN;
    state_dict: the neutral keys convs.I.{weight,bias}.  One features() call is one batch of equally sized images."""

    prefix = "vgg"

    def __init__(self, plan, state_dict: Dict[str, torch.Tensor], dtype: torch.dtype = torch.bfloat16, device: str = "cuda:0",
                 in_channels: int = 3):
        self.L = _lib.lib()
        if not torch.cuda.is_available():
            raise _lib.DsimError("no GPU visible: the VGG engine runs only on the HIP device")
        entries = [0 if e in ("P", "M", 0) else e for e in plan]
        if not all(isinstance(e, int) and not isinstance(e, bool) and e >= 0 for e in entries) or len(entries) >= _lib.VGG_MAX_PLAN:
            raise _lib.DsimError(f"bad VGG plan {list(plan)!r}: conv channels and 'P', fewer than {_lib.VGG_MAX_PLAN} entries")
        self.plan, self.dtype, self.device = tuple(entries), dtype, torch.device(device)
        c = _lib.VGGCfgC()
        c.in_channels, c.compute_dtype = int(in_channels), _TORCH2DSIM.get(dtype, -1)
        for i in range(_lib.VGG_MAX_PLAN):
            c.plan[i] = entries[i] if i < len(entries) else -1
        self.in_channels = int(in_channels)
        self.channels = next((e for e in reversed(entries) if e > 0), 0)
        self._create_and_load(c, state_dict)

    def out_shape(self, H: int, W: int) -> Tuple[int, int, int]:
        """(H', W', C) of the tap for H x W inputs"""
        h, w, ch = C.c_int(), C.c_int(), C.c_int()
        _lib.check(self.L.dsim_vgg_out_shape(self._h, int(H), int(W), C.byref(h), C.byref(w), C.byref(ch)), "dsim_vgg_out_shape")
        return h.value, w.value, ch.value

    def workspace_bytes(self, n_images: int, H: int, W: int) -> int:
        return int(self.L.dsim_vgg_workspace_bytes(self._h, n_images, int(H), int(W)))

    def max_images(self, H: int, W: int, upper: int = 4096) -> int:
        """Largest n_images one features call accepts at H x W (every activation < 2 GiB)."""
        return self._largest(lambda m: self.workspace_bytes(m, H, W) > 0, upper)

    def features(self, pixels: torch.Tensor) -> torch.Tensor:
        """pixels: normalised f32 (n, in_channels, H, W) on the device -> the last conv's output (n, H', W', C), channel-last, in the
        compute dtype, without ReLU."""
        _require_cuda(pixels)
        if pixels.ndim != 4 or pixels.shape[1] != self.in_channels or pixels.dtype != torch.float32 or pixels.shape[0] < 1:
            raise _lib.DsimError(f"pixels must be float32 (n,{self.in_channels},H,W): {tuple(pixels.shape)} {pixels.dtype}")
        n, _, H, W = pixels.shape
        with torch.cuda.device(self.device):
            need = self.workspace_bytes(n, H, W)
            if not need:
                raise _lib.DsimError(f"{n} images of {H}x{W} do not fit one call (smaller than the pools allow, or an activation would "
                                     "reach 2 GiB)")
            ws = self._arena(need)
            out = torch.empty((n,) + self.out_shape(H, W), dtype=self.dtype, device=self.device)
            _lib.check(self.L.dsim_vgg_features(self._h, pixels.data_ptr(), n, H, W, out.data_ptr(), ws.data_ptr(), ws.numel(),
                                                _stream_ptr()), "dsim_vgg_features")
        return out


def gram_rows_workspace_bytes(n: int, P: int, Cc: int, row0: int, n_rows: int, dtype: torch.dtype) -> int:
    return int(_lib.lib().dsim_gram_rows_workspace_bytes(n, P, Cc, row0, n_rows, _TORCH2DSIM.get(dtype, -1)))


def gram_rows(feat: torch.Tensor, row0: int = 0, n_rows: Optional[int] = None):
    """Rows [row0, row0 + n_rows) of each image's Gram matrix (dsim_gram_rows): feat (n, ..., C) channel-last of the three dtypes ->
    (rows f32 (n, n_rows, C), stats f32 (n, 4)), what feature_pair_score / feature_matrix take.  A negative row0 counts from the end."""
    _require_cuda(feat)
    if feat.dtype not in _TORCH2DSIM or feat.ndim < 3:
        raise _lib.DsimError("feat must be contiguous (n, ..., C) of dtype float32, bfloat16 or float16")
    n, Cc = feat.shape[0], feat.shape[-1]
    P = feat[0].numel() // max(Cc, 1)
    row0 = row0 + Cc if row0 < 0 else row0
    n_rows = Cc - row0 if n_rows is None else int(n_rows)
    dt = _TORCH2DSIM[feat.dtype]
    out = torch.empty((n, max(n_rows, 0), Cc), dtype=torch.float32, device=feat.device)
    stats = torch.empty((n, 4), dtype=torch.float32, device=feat.device)
    _tail_call(feat.device, "gram_rows", (n, P, Cc, row0, n_rows, dt), f"no Gram rows for n={n} P={P} C={Cc} rows [{row0}, {row0 + n_rows})",
               feat.data_ptr(), n, P, Cc, row0, n_rows, dt, out.data_ptr(), stats.data_ptr())
    return out, stats


def op_relu(x: torch.Tensor) -> torch.Tensor:
    """relu(x) on the VGG stack's kernel (a copy; the kernel itself works in place)"""
    _require_cuda(x)
    out = x.clone()
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().dsim_op_relu(out.data_ptr(), out.numel(), _TORCH2DSIM.get(x.dtype, -1), _stream_ptr()), "dsim_op_relu")
    return out


def op_relu_pool2(x: torch.Tensor) -> torch.Tensor:
    """maxpool2x2(relu(x)) of channel-last x (n, H, W, C), floor mode, on the VGG stack's kernel"""
    _require_cuda(x)
    n, H, W, Cc = x.shape
    out = torch.empty((n, H // 2, W // 2, Cc), dtype=x.dtype, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().dsim_op_relu_pool2(x.data_ptr(), out.data_ptr(), n, H, W, Cc, _TORCH2DSIM.get(x.dtype, -1), _stream_ptr()),
                   "dsim_op_relu_pool2")
    return out
