"""The executor walks (csrc/unet.hip, csrc/dit.hip, csrc/vae.hip) in their 16-bit modes against float64 at every tap: the references,
the metrics and the bound shared by tests/test_walk64_host.py and tests/test_gpu_walk64.py.  Not a conftest: import it like
tests/_gemm64.py.

WHAT IS COMPARED.  q, k, v of every tap as [B][N][H * D] (B = 2 x images, [image][cfg] order), the VAE moments as [B][HW][C]:

  * ref64: the oracle (oracle/cpu_ref.py) evaluated in float64 on THE NETWORK THE ENGINE HOLDS (engine_weights()).  What the
    handle packs to the compute dtype is rounded to it first, what it keeps in f32 is left as it is.  The split, read from
    store.h pack_all(), unet.hip set_cond(), dit.hip dsim_dit_set_conditioning() and vae.hip dsim_vae_finalize():
      - kept f32: every 1-d tensor (biases, GroupNorm / LayerNorm affines); `conv_in.weight` of the U-Net and of the VAE (the direct
        conv_in kernels read f32 latents / pixels and f32 weights); `time_embedding.*`, `add_embedding.*` and every
        `time_emb_proj.weight` (consumed by gemv_f32 in set_cond, their result an f32 bias of conv1); of the DiT `pos_embed`,
        `x_embedder.proj.weight`, `y_embedder.embedding_table.weight`, `t_embedder.*` and every `adaLN_modulation.1.weight` (f32
        patch embedding, table lookup and GEMVs: the 6 x depth modulation vectors are f32);
      - rounded to the compute dtype: every other 2-d or 4-d tensor (Linear, 1 x 1 and 3 x 3 conv weights -- the GEMM operands);
      - the VAE's quant_conv is folded into conv_out at finalize: W' = RN16(Wq RN16(Wco)) with Wq in f32, b' = Wq bco + bq in f32.
        engine_weights() states the same network: conv_out carries W', b' and quant_conv becomes the identity.
    The inputs likewise: latents, noise and pixels stay f32 (x_t = sa z + sb eps is formed in f32 inside conv_in / the patch
    embedding); the prompt context is converted to the compute dtype on entry and is rounded here; SDXL's pooled embedding and time
    ids stay f32.  No activation is rounded in ref64.
  * ref16: the reference's own 16-bit walk -- the same oracle run natively by torch on the CPU in bf16 / fp16, the module
    cast with .to(dtype) (so the f32-kept tensors are rounded too, as a 16-bit torch pipeline holds them), on the same weights,
    context and inputs.  (fp16 convolutions alone are evaluated as RN16 of the f32 convolution: _conv_through_f32.)  It is the yardstick, not a second reference: how far an honest 16-bit walk of this network lies from ref64.
  * leaf16: float64 with every leaf module's output rounded to the dtype (forward hooks) -- a second honest realisation, used on the
    CPU to show that the bound does not reject honest rounding.

METRICS, per tap and per q, k, v (metrics()):
  rms = ||got - ref64|| / ||ref64||                                       relative RMS error
  row = max_token ||e_row|| / sqrt(mean_token ||ref64_row||^2)            normalised worst token-row error
(rms alone averages one bad row block away: 16 wrong rows of 768 are 2 % of the energy.)

THE BOUND (violations()):  metric(engine) <= MARGIN x metric(ref16), per tap, per tensor, per metric.  The scale comes from the
reference's own 16-bit walk, never from the engine.  MARGIN = 2: two honest rounding realisations of one walk differ by up to about 2 x
(ref16 on leaf16's scale below: 1.6 x in rms; the row metric, a maximum over ~1500 rows, 1.8-2.1 x); the engine rounds at fewer
points than torch (it fuses), so it should sit at or below ref16 -- measured on an MI355X it does: 0.59-1.04 x over every model,
dtype and fusion mask (tests/test_gpu_walk64.py has the table).  MARGIN must stay below 4: above that the weakest bf16 defects below
(the lost time embedding at x 4.9, the row block at x 13) would no longer be certain to fail.  The fp8 (e4m3) attention mode of the
DiT has its own margin over the same ref16 (MARGIN_FP8, tests/test_gpu_walk64.py).

WHAT THE BOUND SEES (tests/test_walk64_host.py prints these; TINY U-Net at a 16 x 16 latent and DIT_TINY, step 600, 3 images, ref16
standing in for the engine, the defect planted with a forward hook; "x f" = the defective walk's worst metric / clean ref16's, the
smallest over the taps behind the defect .. the largest):
                                              bf16                         fp16
  1 a 16-token row block of one FF zeroed     x 13.4 (u0) .. x 44.3 (d0)   x 112 (m)  .. x 379 (d0)
  2 one token row of one image zeroed         x 2.6 (m)   .. x 25.0 (d0)   x 17.7 (m) .. x 214 (d0)
  3 cond / uncond swapped in one attn2        x 17.6 (u0) .. x 35.8 (d0)   x 147 (m)  .. x 287 (d0)
  4 one resnet's time_emb_proj zeroed         x 4.9 (u2)  .. x 8.1 (d1)    x 37.7 (u2) .. x 59.1 (d1)
  5 two skips swapped in one up block         x 12.9 (u2) .. x 21.0 (u0)   x 104 (u2) .. x 173 (u0)
  6 DiT: gate_msa of block 0 set to 1         x 82 .. x 106                x 640 .. x 857
  every tap in front of a defect              x 1.0 exactly                x 1.0 exactly
  leaf16 on ref16's scale (honest)            x 0.5 .. x 0.8               x 0.5 .. x 0.8
  ref16 on leaf16's scale (honest)            rms x 1.57, row x 1.86       rms x 1.65, row x 2.12
In bf16 one zeroed token row (defect 2) clears MARGIN = 2 by little in the middle of the net (x 2.6, x 3.2, x 3.4): bf16's own
rounding (1-2 % rms) is as large as what one row of 256 contributes three blocks later, so the host test asserts it at the first tap
behind the defect only.  fp16 rounds 8 x finer and sees every defect at every tap behind it by a factor of 17 or more -- and the fp16
kernels are the bf16 sources compiled in a namespace, so the per-tap fp16 comparison is the sharp structural test of the bf16 walk
too.  That is why tests/test_gpu_walk64.py runs both dtypes.
"""
import dataclasses

import torch
import torch.nn.functional as F

from diffsim_amd import scheduler as sched

MARGIN = 2.0
STEP = 600
TENSORS = ("q", "k", "v")
METRICS = ("rms", "row")


# ---- the network the engine holds --------------------------------------------------------------------------------------------
_F32_PREFIX = ("time_embedding.", "add_embedding.", "t_embedder.")
_F32_SUFFIX = ("conv_in.weight", "time_emb_proj.weight", "x_embedder.proj.weight", "embedding_table.weight",
               "adaLN_modulation.1.weight")


def engine_keeps_f32(key: str, ndim: int) -> bool:
    """Does the handle keep this parameter in f32 (True) or pack it to the compute dtype (False)?  store.h pack_all()."""
    return ndim == 1 or key == "pos_embed" or key.startswith(_F32_PREFIX) or key.endswith(_F32_SUFFIX)


def engine_weights(sd, dtype):
    """The state dict as the handle holds it, in f32 values: packed tensors rounded to `dtype`, the others untouched; a VAE state
    dict (one with quant_conv) gets conv_out <- the folded conv_out . quant_conv and quant_conv <- the identity."""
    out = {k: (v.float() if engine_keeps_f32(k, v.ndim) else v.to(dtype).float()) for k, v in sd.items()}
    if "quant_conv.weight" in sd:
        f64 = torch.float64
        wq = sd["quant_conv.weight"].to(f64).flatten(1)                   # f32 in the fold (the raw tensor, not the packed one)
        wco = out["encoder.conv_out.weight"].to(f64)
        out["encoder.conv_out.weight"] = torch.einsum("oc,cikl->oikl", wq, wco).to(dtype).float()
        out["encoder.conv_out.bias"] = (wq @ sd["encoder.conv_out.bias"].to(f64) + sd["quant_conv.bias"].to(f64)).float()
        out["quant_conv.weight"] = torch.eye(wq.shape[0]).reshape(sd["quant_conv.weight"].shape).clone()
        out["quant_conv.bias"] = torch.zeros_like(sd["quant_conv.bias"])
    return out


def _conv_through_f32(conv):
    """An fp16 Conv2d as RN16(the f32 convolution of its fp16 operands): the rounding point of a native fp16 convolution with an f32
    accumulator.  torch's own CPU fp16 conv2d has no vectorised path on hosts without AVX512-FP16 (measured 2 s against 1 ms for one
    128-channel 3 x 3 conv at 64 x 64) -- the rest of the fp16 walk (Linear, norms, activations, SDPA, adds) runs natively."""
    def forward(x):
        b = conv.bias
        return F.conv2d(x.float(), conv.weight.float(), None if b is None else b.float(), conv.stride, conv.padding).to(x.dtype)
    conv.forward = forward


def _assign(model, sd, dtype):
    full = {k: (sd[k].to(dtype) if k in sd else torch.zeros(v.shape, dtype=dtype)) for k, v in model.state_dict().items()}
    model.load_state_dict(full, strict=True, assign=True)
    if dtype == torch.float16:
        for m in model.modules():
            if isinstance(m, torch.nn.Conv2d):
                _conv_through_f32(m)
    return model.eval()


def oracle_unet(R, rcfg, sd, shapes=None, dtype=torch.float32):
    """Oracle U-Net without materialising random-init parameters first: meta construction + assign (the unused tail of
    the graph gets zero tensors, which calloc never touches).  `shapes` (the parameter plan some callers hold) is not needed: the
    model's own state dict names every shape."""
    with torch.device("meta"):
        m = R.UNet2DConditionModel(rcfg)
    return _assign(m, sd, dtype)


def oracle_dit(R, rcfg, sd, dtype=torch.float32):
    with torch.device("meta"):
        m = R.DiTOracle(rcfg)
    return _assign(m, sd, dtype)


def oracle_vae(R, rcfg, sd, dtype=torch.float32):
    with torch.device("meta"):
        m = R.AutoencoderKLEncoder(rcfg)
    return _assign(m, sd, dtype)


# ---- oracle forwards that return every tap --------------------------------------------------------------------------------------
def qkv_at_taps(R, unet, x, t, ctx, added, taps):
    """q,k,v of several taps from ONE oracle forward (pre-hooks, diffsim/diffsim.py:43-56 style); stops at the last."""
    store, hooks = {}, []
    names = list(taps)
    for name in names:
        mod = unet.tap_module(*taps[name])

        def hook(m, inp, name=name):
            store[name] = m.qkv(inp[0])
            if name == names[-1]:
                raise R._TapReached()
        hooks.append(mod.register_forward_pre_hook(hook))
    try:
        with torch.no_grad():
            unet.forward(x, t, ctx, None, added)
    except R._TapReached:
        pass
    finally:
        for h in hooks:
            h.remove()
    return store


def tokens(t):
    """the oracle's (B, H, N, D) -> [B][N][H * D] float64, the engine's layout"""
    return t.transpose(1, 2).reshape(t.shape[0], t.shape[2], -1).double()


def dit_qkv_all(model, xt, t_model, num_classes, layers):
    """DiTOracle.qkv_at at every block of `layers` from one forward, in the model's own dtype (the timestep frequencies in f32, as the
    oracle and the engine form them): xt (n, C, S, S) -> {layer: (q, k, v) [2n][N][H * D]}, batch element 2 i + j = image i under
    label [1, null][j] (diffsim_dit.py's batch quirk: one x, two conditionings)."""
    import math
    wd = model.pos_embed.dtype
    n = xt.shape[0]
    te = model.t_embedder
    half = te.fdim // 2
    freqs = torch.exp(-math.log(10000) * torch.arange(half, dtype=torch.float32) / half)
    args = torch.tensor([float(t_model)])[:, None] * freqs[None]
    out = {}
    with torch.no_grad():
        c = te.mlp(torch.cat([torch.cos(args), torch.sin(args)], dim=-1).to(wd)) + model.y_embedder.embedding_table(torch.tensor([1, num_classes]))
        c = c.repeat(n, 1)
        h = model.x_embedder.proj(xt.to(wd)).flatten(2).transpose(1, 2) + model.pos_embed
        h = h.repeat_interleave(2, dim=0)
        for i, blk in enumerate(model.blocks):
            if i in layers:
                sm, cm = blk.adaLN_modulation(c).chunk(6, dim=1)[:2]
                out[i] = tuple(tokens(f) for f in blk.attn.split(blk.norm1(h) * (1 + cm.unsqueeze(1)) + sm.unsqueeze(1)))
            if i == max(layers):
                break
            h = blk(h, c)
    return out


def round_leaves(model, dtype):
    """leaf16: forward hooks that round every leaf module's output to `dtype`; returns the handles (remove() them)."""
    return [m.register_forward_hook(lambda mo, i, o: o.to(dtype).to(o.dtype)) for m in model.modules() if not list(m.children())]


# ---- the walks' inputs, as the scorers form them ------------------------------------------------------------------------------
def unet_batch(cfg, lat, noise, ctxs, pooled=None, step=STEP):
    """(x float64 [2n], t, ctx f32 [2n][L][Dc], added) of the oracle forward over n images in the engine's [image][cfg] order.
    ctxs: one (2, L, Dc) context or a list of n.  pooled: SDXL's (2, P) -> the text_time conditioning and SDXL's input scaling."""
    n = lat.shape[0]
    if pooled is None:
        t = sched.timestep_from_index(step)
        a, b = sched.noise_coefficients(t)
        added = None
    else:
        t, a, b = sched.sdxl_step_coefficients(step)
        side = float(cfg.sample_size * 8)
        ids = torch.tensor([[side, side, 0.0, 0.0, side, side]], dtype=torch.float32)
        added = {"text_embeds": pooled.repeat(n, 1), "time_ids": ids.repeat(2 * n, 1)}
    x = (a * lat.double() + b * noise.double()).repeat_interleave(2, dim=0)
    ctx = ctxs.repeat(n, 1, 1) if torch.is_tensor(ctxs) else torch.cat(list(ctxs))
    return x, t, ctx, added


def unet_walk(R, model, batch, taps, dtype16=None):
    """{tap name: (q, k, v) [B][N][H * D] float64} of one oracle forward in the model's dtype; the context is rounded to dtype16 (the
    engine converts it on entry), the rest of the inputs cast to the model's dtype."""
    x, t, ctx, added = batch
    wd = model.conv_in.weight.dtype
    if dtype16 is not None:
        ctx = ctx.to(dtype16)
    out = qkv_at_taps(R, model, x.to(wd), t, ctx.to(wd), added, taps)
    return {k: tuple(tokens(f) for f in v) for k, v in out.items()}


def vae_moments(model, images):
    """[B][HW][C] float64 moments of the oracle VAE encoder in the model's own dtype"""
    wd = model.quant_conv.weight.dtype
    with torch.no_grad():
        m = model.quant_conv(model.encoder(images.to(wd)))
    return nchw_rows(m)


def nchw_rows(m):
    return m.flatten(2).transpose(1, 2).double()


# ---- metrics and the bound -------------------------------------------------------------------------------------------------------
def metrics(got, ref):
    """(rms, row) of got against ref, both [B][N][C] float64"""
    e = got.double() - ref
    rn = float(ref.norm())
    rows = ref.shape[0] * ref.shape[1]
    return float(e.norm()) / rn, float(e.norm(dim=-1).max()) / (rn / rows ** 0.5)


@dataclasses.dataclass
class Ratio:
    tap: object
    tensor: str
    metric: str
    got: float          # the walk under test against ref64
    scale: float        # ref16 against ref64
    ratio: float = 0.0

    def __post_init__(self):
        self.ratio = self.got / self.scale if self.scale > 0 else float("inf")

    def __str__(self):
        return f"{self.tap} {self.tensor} {self.metric}: {self.got:.3e} against ref16's {self.scale:.3e} (x {self.ratio:.2f})"


def ratios(got, ref16, ref64):
    """Every (tap, tensor, metric) of `got` against the scale ref16 sets: got, ref16, ref64 = {tap: tuple of [B][N][C]}."""
    out = []
    for tap in ref64:
        names = TENSORS if len(ref64[tap]) == 3 else tuple(f"t{i}" for i in range(len(ref64[tap])))
        for name, g, r16, r64 in zip(names, got[tap], ref16[tap], ref64[tap]):
            assert tuple(g.shape) == tuple(r64.shape), (tap, name, tuple(g.shape), tuple(r64.shape))
            for mname, a, b in zip(METRICS, metrics(g, r64), metrics(r16, r64)):
                out.append(Ratio(tap, name, mname, a, b))
    return out


def violations(rs, margin=MARGIN):
    """the entries of ratios() over the bound metric(got) <= margin x metric(ref16); a non-finite value is one"""
    return [r for r in rs if not (r.got <= margin * r.scale)]


def worst(rs, tap=None):
    """the largest ratio (of one tap, or of all)"""
    return max((r.ratio for r in rs if tap is None or r.tap == tap), default=0.0)
