"""Command-line driver: the reference's benchmark loops on the MI355X engine.

``python -m diffsim_amd --dataset cute|nights|sref --metric diffsim|diffsim_xl|dit|clip_cross|dino_cross|diffeats|dinofeats|gram --model_path <dir> --image_path <dir> ...``

Flags of the reference drivers (``/root/reference/argprocess.py:5-18``) keep their names, meaning and defaults;
``--dataset`` selects which of the reference's loops runs (``cute_main.py:48-226``, ``night_main.py:24-173`` or
``style_main.py:24-196`` -- separate scripts there), ``--model_path / --dtype / --batch / --unet_batch / --ngpu / --noise_dtype / --gpu_resize / --mask_path / --query_mask_path / --gallery_mask_path / --save_region_maps / --save_region_matches / --text_attn / --text_threshold / --soft_masks / --text_soft / --transfer_masks / --transfer_threshold / --save_transfer`` are additions of this build (the reference
hard-codes NAS checkpoint paths, ``cute_main.py:25-31``, fp16 and one GPU, ``cute_main.sh:1``).

Multi-GPU (``--ngpu N``): the parent starts N rank processes before anything touches the GPU; triplets are sharded
whole over ranks and the per-triplet scores are all-gathered (RCCL) -- rank 0 prints the accuracy.
"""
from __future__ import annotations

import argparse
import os
import random
import sys
from typing import List, Optional, Tuple

METRICS = ["diffsim", "diffsim_xl", "clip_i", "clip_cross", "dino", "dinov1", "dino_cross", "cute", "lpips", "gram",
           "diffeats", "clipfeats", "dinofeats", "ensemble", "dit"]
ENGINE_METRICS = ("diffsim", "diffsim_xl", "dit", "clip_cross", "dino_cross", "diffeats", "dinofeats", "gram")
VIT_METRICS = ("clip_cross", "dino_cross")      # DiffSim's method on a ViT tower (vit.py): no VAE, no noise, no prompt, no token grid
FEATURE_METRICS = ("diffeats", "dinofeats")     # the cosine of the tapped layer's own features (feats.py), the paper's ablation
GRAM_METRIC = "gram"                            # the VGG-19 Gram style baseline (gram.py): no VAE, noise, prompt, taps or tokens


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="python -m diffsim_amd", description="DiffSim scoring (MI355X-native engine)", allow_abbrev=False)
    p.add_argument("--image_path", type=str, help="Path to image folder")
    p.add_argument("--original_path", type=str, default=None, help="Path to original images for ipref")
    p.add_argument("--out_path", type=str, help="Path to the output folder")
    p.add_argument("--image_size", type=int, default=512, help="(Resized) resolution of compared image")
    p.add_argument("--target_block", type=str, choices=["down_blocks", "mid_blocks", "up_blocks"], default="up_blocks")
    p.add_argument("--target_layer", type=int, default=2, nargs="+")
    p.add_argument("--target_step", type=int, default=100)
    p.add_argument("--metric", type=str, default="diffsim", choices=METRICS)
    p.add_argument("--similarity", type=str, choices=["cosine", "mse"], default="mse")
    p.add_argument("--prompt", type=str, default="High quality image")
    p.add_argument("--ip_adapter", action="store_true")
    p.add_argument("--use_mask", action="store_true")
    p.add_argument("--use_text_attn", action="store_true")
    p.add_argument("--seed", type=int, default=2333)
    # additions of this build
    p.add_argument("--dataset", type=str, choices=["cute", "nights", "sref", "retrieval"], default="cute",
                   help="which reference loop to run: cute_main.py (class/instance/lighting tree), night_main.py (data.csv) or "
                        "style_main.py (Sref / InstantStyle: one folder per style, 2000 sampled experiments); retrieval: every "
                        "--query_path image against every --image_path (gallery) image, top-k rankings written to --out_path (one .txt per "
                        "query, named by its path under --query_path)")
    p.add_argument("--query_path", type=str, default=None, help="--dataset retrieval: folder of query images")
    p.add_argument("--topk", type=int, default=10, help="--dataset retrieval: gallery entries ranked per query")
    p.add_argument("--save_maps", action="store_true",
                   help="--dataset retrieval: beside each ranking .txt also write <name>.npz with the similarity maps of the query "
                        "against its top-k gallery images (gallery, score (k,), local and contrib (k, 2, h, w): direction 0 on the "
                        "query's token grid, 1 on the gallery image's)")
    p.add_argument("--save_matches", action="store_true",
                   help="--dataset retrieval: beside each ranking .txt also write <name>.match.npz with the token alignments of the "
                        "query against its top-k gallery images (gallery, match and weight (k, 2, h, w), expect (k, 2, h, w, 2): "
                        "direction 0 on the query's token grid pointing into the gallery image's, 1 the other way round)")
    p.add_argument("--save_region_maps", action="store_true",
                   help="--dataset retrieval with --query_mask_path / --gallery_mask_path: beside each ranking .txt also write "
                        "<name>.npz with the REGION maps of the query against its top-k gallery images: --save_maps' arrays computed "
                        "over the masked tokens alone (the terms of the region score; zeros at the off tokens), and mask (k, 2, h, w)")
    p.add_argument("--save_region_matches", action="store_true",
                   help="--dataset retrieval with --query_mask_path / --gallery_mask_path: beside each ranking .txt also write "
                        "<name>.match.npz with the REGION alignments of the query against its top-k gallery images: --save_matches' "
                        "arrays with every softmax over the other image's masked tokens alone (off tokens: match -1, weight 0, expect "
                        "(-1, -1)), and mask (k, 2, h, w)")
    p.add_argument("--taps", type=str, nargs="+", default=None, metavar="SPEC",
                   help="--dataset cute|nights|sref: score every tap from one forward per image batch instead of the one "
                        "--target_block / --target_layer tap (which it overrides), and print one section per tap, in the given "
                        "order, as a one-tap run prints it.  SPEC: diffsim up_blocks:0, down_blocks:2, mid_blocks:0; diffsim_xl "
                        "up_blocks:0,1,9 (block, attention, transformer block), mid_blocks:0,5; dit blocks:13; clip_cross / dino_cross layers:5.  Layers are "
                        "explicit (no coercion of a single value to 0).  `all`: every tap the model can name")
    p.add_argument("--mask_path", type=str, default=None, metavar="DIR",
                   help="--dataset cute|nights: score the masked part of each image (region scores).  The mask of "
                        "<image_path>/rel/name.ext is <DIR>/rel/name.png, else <DIR>/rel/name.ext (any mode; area-averaged onto the "
                        "tap's token grid, a token on at >= 128); an image without a mask file is scored whole, and the run prints "
                        "how many were.  Implies --use_mask")
    p.add_argument("--query_mask_path", type=str, default=None, metavar="DIR",
                   help="--dataset retrieval: rank by the masked part of each query image (a region score matrix).  The mask of "
                        "<query_path>/rel/name.ext is <DIR>/rel/name.png, else <DIR>/rel/name.ext (as --mask_path reads them); a query "
                        "without a mask file is scored whole, and the run prints how many were.  May be given without "
                        "--gallery_mask_path: the gallery images are then whole")
    p.add_argument("--gallery_mask_path", type=str, default=None, metavar="DIR",
                   help="--dataset retrieval: the same for the gallery images under --image_path.  May be given without "
                        "--query_mask_path")
    p.add_argument("--text_attn", type=str, nargs="*", default=None, metavar="WORD",
                   help="--dataset cute|nights, --metric diffsim|diffsim_xl: score the part of each image the prompt names "
                        "(text-guided regions).  Each image's region is the tokens whose cross-attention to the WORDs of its row's "
                        "prompt (no WORD: every content token of the prompt) is at least --text_threshold x the image's mean; the "
                        "run prints the mean share of tokens on.  Implies --use_text_attn")
    p.add_argument("--soft_masks", action="store_true",
                   help="--mask_path: soft region scores -- a mask's area average on the token grid is the token's weight (0 .. 255) "
                        "instead of being thresholded at 128, so a partly covered token counts partly, in both attentions and in the "
                        "sums.  Masks of 0 and 255 alone on the grid give the --mask_path scores.  With --dataset retrieval and "
                        "--query_mask_path / --gallery_mask_path: the soft score matrix; the run prints the mean token weight per side")
    p.add_argument("--text_soft", action="store_true",
                   help="--text_attn: soft text-guided regions -- a token below --text_threshold x the mean saliency keeps its share of "
                        "the threshold as a weight instead of being switched off; the run prints the mean token weight")
    p.add_argument("--text_threshold", type=float, default=1.0,
                   help="--text_attn: a token is in its image's region at >= this multiple of the image's mean text saliency "
                        "(0: every token; a region with no token on is the whole image)")
    p.add_argument("--transfer_masks", action="store_true", default=argparse.SUPPRESS,      # (off: _Args.transfer_masks)
                   help="--dataset retrieval with --query_mask_path: exemplar-guided retrieval -- only the queries read their mask "
                        "files; every gallery image's region against a query is the tokens whose attention mass into the query's masked "
                        "tokens passes --transfer_threshold, and the ranking is by the region score of each cell.  "
                        "--mask_path, --dataset cute|nights, --metric diffsim|diffsim_xl|dit: exemplar-guided regions -- only the "
                        "reference image of each triplet reads its mask file; each candidate's region is the tokens whose attention mass "
                        "into the reference's masked tokens is at least --transfer_threshold x the candidate's mean mass.  With "
                        "--soft_masks the reference's weights and the transferred regions are soft.  The run prints how many references "
                        "had no mask file and the mean share of tokens on")
    p.add_argument("--transfer_threshold", type=float, default=argparse.SUPPRESS, metavar="T",      # (default: _Args.transfer_threshold)
                   help="--transfer_masks: a candidate's token is in its region at >= this multiple of the image's mean attention mass "
                        "(default 1.0; 0: every token; a region with no token on is the whole image)")
    p.add_argument("--save_transfer", action="store_true", default=argparse.SUPPRESS,      # (off: _Args.save_transfer)
                   help="--dataset retrieval with --transfer_masks: beside each ranking .txt also write <name>.transfer.npz with the "
                        "regions the query's mask transferred to its top-k gallery images (gallery, region (k, h, w), bool or with "
                        "--soft_masks uint8 weights, and mass (k, h, w), the attention mass on each gallery image's token grid)")
    p.add_argument("--experiments", type=int, default=2000, help="--dataset sref: sampled experiments (style_main.py:64)")
    p.add_argument("--model_path", type=str, default=None, help="diffusers-layout checkpoint directory (unet/, vae/, text_encoder/, tokenizer/)")
    p.add_argument("--dtype", type=str, choices=["bf16", "fp16", "fp32"], default="bf16",
                   help="engine compute dtype (fp16 = the reference drivers' torch.float16; fp32 = parity mode)")
    p.add_argument("--noise_dtype", type=str, choices=["fp32", "fp16"], default="fp32",
                   help="generator draws / add_noise arithmetic: fp32 pipeline or the reference's literal fp16 pipeline")
    p.add_argument("--batch", type=int, default=10, help="triplets per decode / VAE-encode chunk")
    p.add_argument("--unet_batch", type=int, default=None,
                   help="triplets per U-Net engine batch (default: chosen from free device memory; lower it on a shared or smaller GPU)")
    p.add_argument("--ngpu", type=int, default=None,
                   help="GPUs of this node to shard the triplets over (one process each); default 1, or the launcher's rank count")
    p.add_argument("--decode_procs", type=str, default="auto",
                   help="worker processes that decode + resize the image files ahead of the GPU: a number, 0 = threads of this "
                        "process, auto = host cores / ranks of the node")
    p.add_argument("--gpu_resize", action="store_true", default=argparse.SUPPRESS,      # (off: _Args.gpu_resize)
                   help="decode the image files on the host and resize them on the GPU (PIL's Lanczos / bicubic arithmetic, bit for "
                        "bit: the same scores); images outside the served range are resized by PIL on the host")
    p.add_argument("--fp8_attention", action="store_true", help="--metric dit: e4m3 MFMA attention")
    p.add_argument("--gram_full", action="store_true", default=argparse.SUPPRESS,      # (off: _Args.gram_full)
                   help="--metric gram: the cosine of the whole 512 x 512 Gram matrices instead of the reference's, which is the cosine "
                        "of their last rows (vgg_gram.py:81 indexes a tensor with [-1])")
    p.add_argument("--dedup_cfg", dest="dedup_cfg", action="store_true", default=True,
                   help="--metric diffsim: compute what the two CFG halves share once per image (bit-identical scores, ~6 %% faster); the default")
    p.add_argument("--selftest_shard", action="store_true",
                   help="CPU-only check of the N-rank triplet sharding: the dataset walk, the strided shard, the two score gathers and "
                        "the printed counts over gloo with a stand-in scorer (no GPU, no weights)")
    p.add_argument("--no_dedup_cfg", dest="dedup_cfg", action="store_false",
                   help="--metric diffsim: run the reference's duplicated CFG batch through every layer")
    return p


class _Args(argparse.Namespace):
    """The parsed flags.  An opt-in switch that is off reads False from here and is no entry of the namespace, so that an argument
    list without it parses to exactly the namespace it parsed to before the switch existed."""
    gpu_resize = False
    transfer_masks = False
    transfer_threshold = 1.0
    save_transfer = False
    gram_full = False


def arg_parse(argv=None):
    p = build_parser()
    args = p.parse_args(argv, namespace=_Args())
    soft_matrix = args.soft_masks and args.dataset == "retrieval"       # the soft score matrix: its masks are the two sets' own
    for flag, on, partner, has in (("--soft_masks", args.soft_masks and not soft_matrix, "--mask_path", args.mask_path is not None),
                                   ("--text_soft", args.text_soft, "--text_attn", args.text_attn is not None)):
        if not on:
            continue
        if not has:
            p.error(f"{flag} weighs the tokens of {partner}: it needs {partner}")
        if args.dataset == "retrieval" or args.taps is not None:
            p.error(f"{flag} scores soft regions on the one-tap triplet benchmarks (--dataset cute or nights): "
                    + ("--dataset retrieval (text-guided retrieval) and " if flag == "--text_soft" else "")
                    + "a sweep (--taps) " + ("are" if flag == "--text_soft" else "is") + " not supported with it")
        if args.metric in VIT_METRICS or args.metric in FEATURE_METRICS:
            p.error(f"{flag}: --metric {args.metric} has no regions")
    if soft_matrix:
        if args.query_mask_path is None and args.gallery_mask_path is None:
            p.error("--soft_masks with --dataset retrieval weighs the tokens of --query_mask_path / --gallery_mask_path (the soft "
                    "score matrix): it needs one of them or both (--mask_path is the triplet benchmarks')")
        if args.metric in VIT_METRICS or args.metric in FEATURE_METRICS:
            p.error(f"--soft_masks: --metric {args.metric} has no regions")
    if "transfer_threshold" in vars(args) and not args.transfer_masks:
        p.error("--transfer_threshold is the threshold of --transfer_masks: it needs --transfer_masks")
    if args.save_transfer and not (args.transfer_masks and args.dataset == "retrieval"):
        p.error("--save_transfer writes the transferred regions of an exemplar-guided retrieval run: it needs --transfer_masks and "
                "--dataset retrieval")
    if args.transfer_masks:
        if args.dataset == "retrieval":
            if args.query_mask_path is None:
                p.error("--transfer_masks with --dataset retrieval transfers the query images' masks to every gallery image: it needs "
                        "--query_mask_path (--mask_path is the triplet benchmarks')")
            if args.gallery_mask_path is not None:
                p.error("--transfer_masks: the gallery's regions are the transferred ones, --gallery_mask_path is not supported with it")
            if args.save_region_maps or args.save_region_matches:
                p.error("--transfer_masks: region maps and region alignments over transferred regions (--save_region_maps, "
                        "--save_region_matches) are not supported")
        elif args.mask_path is None:
            p.error("--transfer_masks transfers the reference images' masks of --mask_path: it needs --mask_path")
        if args.dataset not in ("cute", "nights", "retrieval") or args.taps is not None:
            p.error("--transfer_masks scores exemplar-guided regions on the one-tap triplet benchmarks (--dataset cute or nights, with "
                    "--mask_path) and on retrieval rankings (--dataset retrieval, with --query_mask_path): --dataset sref and a sweep "
                    "(--taps) are not supported with it")
        if args.text_attn is not None:
            p.error("--transfer_masks: an exemplar-guided region and a text-guided region (--text_attn), one or the other")
        if args.metric in VIT_METRICS or args.metric in FEATURE_METRICS:
            p.error(f"--transfer_masks: --metric {args.metric} has no regions")
        if not (args.transfer_threshold >= 0.0) or args.transfer_threshold == float("inf"):
            p.error("--transfer_threshold must be finite and >= 0")
    if args.gram_full and args.metric != GRAM_METRIC:
        p.error("--gram_full chooses the whole Gram matrices of --metric gram: it needs --metric gram")
    if args.metric == GRAM_METRIC:
        if args.similarity != "cosine":
            p.error("--metric gram needs --similarity cosine: its score is always a cosine, as in the reference, and the mse counting "
                    "rule would read it backwards")
        for flag, on in (("--mask_path", args.mask_path is not None), ("--query_mask_path", args.query_mask_path is not None),
                         ("--gallery_mask_path", args.gallery_mask_path is not None), ("--soft_masks", args.soft_masks),
                         ("--save_region_maps", args.save_region_maps), ("--save_region_matches", args.save_region_matches)):
            if on:
                p.error(f"{flag}: --metric gram has no regions (a Gram matrix sums over every position of the image)")
        for flag, on in (("--save_maps", args.save_maps), ("--save_matches", args.save_matches)):
            if on:
                p.error(f"{flag}: --metric gram has no similarity maps or token alignments (its descriptor has no spatial axis)")
        if args.taps is not None:
            p.error("--taps: --metric gram has one tap, conv5_1 of VGG-19 (vgg_gram.py:39); there is nothing to sweep")
        if args.text_attn is not None or args.text_soft:
            p.error("--text_attn: --metric gram has no prompt and no cross-attention, so no text-guided regions")
        if args.transfer_masks:
            p.error("--transfer_masks: --metric gram has no regions, so no exemplar-guided ones")
        if args.fp8_attention:
            p.error("--fp8_attention: --metric gram has no attention (--metric dit only)")
        if args.ngpu is not None and args.ngpu > 1:
            p.error("--metric gram is single-GPU for now: run it with --ngpu 1")
    if args.metric in FEATURE_METRICS:
        if args.similarity != "cosine":
            p.error(f"--metric {args.metric} needs --similarity cosine: its score is always a cosine, as in the reference (which "
                    "ignores the flag), and the mse counting rule would read it backwards")
        for flag, on in (("--mask_path", args.mask_path is not None), ("--query_mask_path", args.query_mask_path is not None),
                         ("--gallery_mask_path", args.gallery_mask_path is not None), ("--text_attn", args.text_attn is not None),
                         ("--save_maps", args.save_maps), ("--save_matches", args.save_matches),
                         ("--save_region_maps", args.save_region_maps), ("--save_region_matches", args.save_region_matches),
                         ("--fp8_attention", args.fp8_attention)):
            if on:
                p.error(f"{flag}: --metric {args.metric} is the plain cosine of the tapped layer's features: it has no regions, maps, "
                        "alignments or fp8 attention")
    region_out =[f for f, on in (("--save_region_maps", args.save_region_maps), ("--save_region_matches", args.save_region_matches)) if on]
    for flag in region_out:
        if args.dataset != "retrieval" or (args.query_mask_path is None and args.gallery_mask_path is None):
            p.error(f"{flag} writes the per-token outputs of region rankings: it needs --dataset retrieval and --query_mask_path and / "
                    "or --gallery_mask_path")
        if args.metric in VIT_METRICS:
            p.error(f"{flag}: --metric {args.metric} has no regions, maps or alignments (its tokens are a class token and a patch grid: "
                    "the class token is not on the grid)")
        if args.taps is not None or args.text_attn is not None:
            p.error(f"{flag} takes one tap (--target_block / --target_layer) and mask files: --taps and --text_attn are not supported "
                    "with it")
    if args.taps is not None:
        if args.dataset == "retrieval" or args.save_maps or args.save_matches:
            p.error("--taps sweeps the triplet benchmarks (--dataset cute, nights or sref): score matrices, similarity maps and "
                    "token alignments (--dataset retrieval, --save_maps, --save_matches) take one tap, --target_block / --target_layer")
        from .sweep import parse_tap_specs
        try:
            parse_tap_specs(args.taps, args.metric)
        except ValueError as e:
            p.error(f"--taps: {e}")
    if args.mask_path is not None:
        if args.dataset not in ("cute", "nights") or args.taps is not None:
            p.error("--mask_path scores regions on the one-tap triplet benchmarks (--dataset cute or nights): a region score matrix "
                    "(--dataset retrieval) takes its masks from --query_mask_path / --gallery_mask_path; --dataset sref and a region "
                    "sweep (--taps) are not supported")
        args.use_mask = True
    for flag in ("query_mask_path", "gallery_mask_path"):
        if getattr(args, flag) is None:
            continue
        if args.dataset != "retrieval":
            p.error(f"--{flag} masks the images of a region score matrix: it needs --dataset retrieval (the triplet benchmarks take "
                    "--mask_path)")
        if args.save_maps or args.save_matches:
            p.error(f"--{flag}: --save_maps and --save_matches write per-token outputs of whole images (their epilogue stores rows in "
                    "order) and are not supported with region rankings; --save_region_maps and --save_region_matches write the "
                    "regions' own")
        if args.text_attn is not None:
            p.error(f"--{flag}: text-guided regions (--text_attn) are not supported for --dataset retrieval")
    if args.text_attn is not None:
        if args.dataset not in ("cute", "nights") or args.taps is not None or args.mask_path is not None:
            p.error("--text_attn scores text-guided regions on the one-tap triplet benchmarks (--dataset cute or nights): "
                    "--dataset retrieval, --dataset sref, a sweep (--taps) and mask files (--mask_path) are not supported with it")
        if args.metric == "dit":
            p.error("--text_attn: --metric dit has no text conditioning (a class-conditional model without cross-attention)")
        if not (args.text_threshold >= 0.0) or args.text_threshold == float("inf"):
            p.error("--text_threshold must be finite and >= 0")
        args.use_text_attn = True
    if args.metric in VIT_METRICS:
        for flag, on in (("--mask_path", args.mask_path is not None), ("--query_mask_path", args.query_mask_path is not None),
                         ("--gallery_mask_path", args.gallery_mask_path is not None), ("--text_attn", args.text_attn is not None),
                         ("--save_maps", args.save_maps), ("--save_matches", args.save_matches)):
            if on:
                p.error(f"{flag}: --metric {args.metric} has no regions, maps or alignments (its tokens are a class token and a "
                        "patch grid: the class token is not on the grid)")
        if args.fp8_attention:
            p.error(f"--fp8_attention: --metric {args.metric} has no fp8 attention (--metric dit only)")
        if args.metric == "clip_cross" and args.dataset == "retrieval":
            p.error("--metric clip_cross --dataset retrieval: clip_cross applies the layer's out_proj in its score tail and there is "
                    "no projected score matrix yet; --metric dino_cross ranks with the plain score matrix")
    if args.save_maps and args.dataset != "retrieval":
        p.error("--save_maps writes the maps of the retrieval rankings: it needs --dataset retrieval")
    if args.save_matches and args.dataset != "retrieval":
        p.error("--save_matches writes the token alignments of the retrieval rankings: it needs --dataset retrieval")
    return args


# ---- the CUTE triplet walk (cute_main.py:48-108) ------------------------------------------------------------------
def cute_triplets(image_path: str, seed: int) -> List[Tuple[str, str, str, str]]:
    """(A, B, C, prompt) in the order the reference's loop visits them: for every class, 10 experiments, every
    instance folder: a random lighting, two random images of it (A, B), one image of another instance under the
    same lighting (C).  The same ``random`` call sequence as the reference (scoring consumes no ``random`` state there,
    so collecting the triplets first is equivalent)."""
    random.seed(seed)
    out = []
    ext = (".png", ".jpg", ".jpeg")
    for cls in os.listdir(image_path):
        if cls == "main.py" or cls == ".DS_Store":
            continue
        cls_dir = os.path.join(image_path, cls)
        for _ in range(10):
            for sub1, dirs2, _files in os.walk(cls_dir):
                for d2 in dirs2:
                    d2_path = os.path.join(sub1, d2)
                    subs3 = [d for d in os.listdir(d2_path) if os.path.isdir(os.path.join(d2_path, d))]
                    if not subs3:
                        continue
                    sel3 = random.choice(subs3)
                    sel3_path = os.path.join(d2_path, sel3)
                    files = [f for f in os.listdir(sel3_path) if f.endswith(ext)]
                    if len(files) < 2:
                        continue
                    a, b = random.sample(files, 2)
                    others = [d for d in dirs2 if d != d2]
                    if not others:
                        continue
                    other3 = os.path.join(sub1, random.choice(others), sel3)
                    ofiles = [f for f in os.listdir(other3) if f.endswith(ext)]
                    if not ofiles:
                        continue
                    c = random.choice(ofiles)
                    out.append((os.path.join(sel3_path, a), os.path.join(sel3_path, b), os.path.join(other3, c),
                                f"The photo of a {cls}"))
    return out


# ---- the Sref / InstantStyle walk (style_main.py:48-76) ----------------------------------------------------------------
def sref_triplets(image_path: str, seed: int, prompt: str, experiments: int = 2000) -> List[Tuple[str, str, str, str]]:
    """(A, B, C, prompt) of the style benchmark: every sub-folder with at least two images is a style; each experiment
    draws two different styles, two images of the first (A, B) and one of the second (C).  The ``random`` calls are the
    reference's, in its order (seeded like it, style_main.py:27), so the same tree gives the same experiments."""
    random.seed(seed)
    ext = (".png", ".jpg", ".jpeg")
    styles = {}
    for root, dirs, _files in os.walk(image_path):
        for d in dirs:
            full = os.path.join(root, d)
            ims = [os.path.join(full, f) for f in os.listdir(full) if f.endswith(ext)]
            if len(ims) >= 2:
                styles[full] = ims
    names = list(styles.keys())
    out = []
    for _ in range(experiments):
        if len(names) < 2:
            continue
        dir_a, dir_c = random.sample(names, 2)
        a, b = random.sample(styles[dir_a], 2)
        c = random.choice(styles[dir_c])
        out.append((a, b, c, prompt))
    return out


def cute_counts(s_ab, s_ac, similarity: str) -> Tuple[int, int]:
    """correct / correct_2x of cute_main.py:196-205 (a NaN score compares False: counted wrong, as there)."""
    if similarity == "mse":
        return int((s_ab < s_ac).sum()), int((s_ab * 2 < s_ac).sum())
    return int((s_ab > s_ac).sum()), int((s_ab > 2 * s_ac).sum())


def build_scorer(args):
    """Flags -> scorer object (DiffSim / diffsim_xl / diffsim_DiT): the object graph of cute_main.py:25-31."""
    import torch
    from . import loader
    if args.metric not in ENGINE_METRICS:
        raise SystemExit(f"--metric {args.metric}: only the DiffSim metrics (diffsim, diffsim_xl, dit, clip_cross, dino_cross) run on "
                         f"this engine; the competitor metrics of the reference are out of scope")
    if args.ip_adapter:
        raise SystemExit("--ip_adapter: IP-Adapter mode is out of scope of this build")
    if not args.model_path:
        raise SystemExit("--model_path is required (no checkpoint is bundled)")
    nd = torch.float16 if args.noise_dtype == "fp16" else torch.float32
    dev = "cuda:%d" % int(os.environ.get("LOCAL_RANK", "0"))
    if args.metric in VIT_METRICS:
        print(f"--metric {args.metric}: --image_size is not consulted (the model's image processor decides: resize, then a centre crop)")
        return (loader.load_clip_cross if args.metric == "clip_cross" else loader.load_dino_cross)(args.model_path, args.dtype, dev)
    if args.metric == GRAM_METRIC:
        print(f"--metric gram: the cosine of the {'whole Gram matrices' if args.gram_full else 'last rows of the Gram matrices (the reference)'}"
              f" of VGG-19 conv5_1; images keep their aspect ratio at --image_size {args.image_size}")
        return loader.load_vgg_gram(args.model_path, args.dtype, dev)
    if args.metric == "dinofeats":
        from .feats import FeatureView
        print("--metric dinofeats: --image_size is not consulted (the model's image processor decides: resize, then a centre crop)")
        return FeatureView(loader.load_dino_cross(args.model_path, args.dtype, dev))
    if args.metric == "diffeats":
        from .feats import FeatureView
        print("--metric diffeats: --target_layer N is taken literally, as in the reference (--metric diffsim turns a single value "
              "into layer 0)")
        return FeatureView(loader.load_diffsim(args.model_path, args.dtype, dev, nd, dedup_cfg=args.dedup_cfg))
    if args.metric == "diffsim":
        return loader.load_diffsim(args.model_path, args.dtype, dev, nd, dedup_cfg=args.dedup_cfg)
    if args.metric == "diffsim_xl":
        return loader.load_diffsim_xl(args.model_path, args.dtype, dev, nd)
    return loader.load_diffsim_dit(args.model_path, args.image_size, args.target_step, args.dtype, dev, args.fp8_attention)


def _selftest_scores(trip, rank, world):
    """Stand-in for harness.score_path_triplets on CPU (--selftest_shard): every rank scores ITS strided shard of the triplets with
    a deterministic function of the file names, then the same two gathers as the real path.  DSIM_SELFTEST_DIE_RANK=r makes
    rank r exit 9 between the two collectives (the supervising launcher must stop the others, which are then waiting in the second)."""
    import torch
    from . import parallel as P

    def fake(a, b):
        return ((sum(map(ord, os.path.basename(a))) * 31 + sum(map(ord, os.path.basename(b))) * 17) % 997) / 997.0
    mine = P.shard_triplets(len(trip), rank, world)
    loc_ab = torch.tensor([fake(trip[j][0], trip[j][1]) for j in mine], dtype=torch.float32)
    loc_ac = torch.tensor([fake(trip[j][0], trip[j][2]) for j in mine], dtype=torch.float32)
    s_ab = P.gather_scores(loc_ab, len(trip), rank, world)
    if os.environ.get("DSIM_SELFTEST_DIE_RANK") == str(rank):
        sys.exit(9)
    s_ac = P.gather_scores(loc_ac, len(trip), rank, world)
    return s_ab, s_ac, 0


def _selftest_scores_taps(trip, rank, world, n_taps):
    """--selftest_shard --taps: _selftest_scores per tap (a deterministic function of the file names and the tap's position),
    the same shard, one pair of gathers per tap."""
    import torch
    from . import parallel as P

    def fake(a, b, t):
        s = ((sum(map(ord, os.path.basename(a))) * 31 + sum(map(ord, os.path.basename(b))) * 17) % 997) / 997.0
        return 1.0 - s if t % 2 else s          # odd taps rank the other way: each tap's section shows its own gathered scores
    mine = P.shard_triplets(len(trip), rank, world)
    s_ab, s_ac = [], []
    for t in range(n_taps):
        loc_ab = torch.tensor([fake(trip[j][0], trip[j][1], t) for j in mine], dtype=torch.float32)
        loc_ac = torch.tensor([fake(trip[j][0], trip[j][2], t) for j in mine], dtype=torch.float32)
        s_ab.append(P.gather_scores(loc_ab, len(trip), rank, world))
        s_ac.append(P.gather_scores(loc_ac, len(trip), rank, world))
    return torch.stack(s_ab), torch.stack(s_ac), [0] * n_taps


def cli_taps(args, scorer):
    """--taps -> the scorer's taps (``all``: every tap of the scorer's model; the default model of --metric without a scorer)."""
    from . import config as C
    from .sweep import parse_tap_specs
    cfg = getattr(scorer, "cfg", None) or {"diffsim": C.SD15, "diffsim_xl": C.SDXL, "dit": C.DIT_XL2, "clip_cross": C.CLIP_B32,
                                           "dino_cross": C.DINOV2_S14, "diffeats": C.SD15, "dinofeats": C.DINOV2_S14}[args.metric]
    try:
        return parse_tap_specs(args.taps, args.metric, cfg)
    except ValueError as e:
        raise SystemExit(f"--taps: {e}")


def _report(args, trip, rows, s_ab, s_ac, bad):
    """The result lines of one tap (rank 0)."""
    from . import harness as H
    total = len(trip)
    if bad:
        print(f"WARNING: {bad} pair score(s) are NaN/inf (counted as wrong, as the reference's comparisons would)")
    if args.dataset == "nights":
        acc = H.nights_accuracy(s_ab, s_ac, [r["vote"] for r in rows], args.similarity)
        print(f"Final validation accuracy: {acc:.2f}%")
    else:
        correct, correct2 = cute_counts(s_ab.cpu(), s_ac.cpu(), args.similarity)
        if total > 0 and args.dataset == "sref":           # style_main.py:186-193
            print(f"Total comparisons: {total}")
            print(f"Accuracy: {correct / total * 100:.2f}%")
            print(f"2x Accuracy: {correct2 / total * 100:.2f}%")
        elif total > 0:                                     # cute_main.py:216-224
            print(f"Total comparisons: {total}")
            print(f"Total {total}; Correct {correct}; Correct 2x {correct2}")
            print(f"Accuracy: {correct / total * 100}%")
            print(f"2x Accuracy: {correct2 / total * 100}%")
        else:
            print("Total comparisons: 0")
            print("No valid comparisons were made.")


def _resize_report(args, rank):
    """--gpu_resize: how many images of this rank took the device resize and how many fell back to PIL (rank 0 prints its own)."""
    if getattr(args, "gpu_resize", False) and rank == 0 and not args.selftest_shard:
        from .engine import RESIZE_COUNTS
        print(f"GPU resize: {RESIZE_COUNTS['gpu']} image(s) resized on the device, {RESIZE_COUNTS['fallback']} fell back to the host")


def run(args) -> int:
    import torch
    from . import harness as H
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1 and args.selftest_shard:
        import torch.distributed as dist
        dist.init_process_group("gloo")
    elif world > 1:
        import torch.distributed as dist
        from .parallel import pin_to_gpu_numa
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
        pin_to_gpu_numa(int(os.environ.get("LOCAL_RANK", "0")))       # image decode threads next to this rank's GPU
        dist.init_process_group("nccl")
    os.environ.setdefault("DSIM_DECODE_PROCS", str(args.decode_procs))      # the scorers' DecodePool default
    scorer = None if args.selftest_shard else build_scorer(args)
    if getattr(args, "gpu_resize", False) and scorer is not None:         # (a plain Namespace without the flag: off)
        getattr(scorer, "scorer", scorer).gpu_resize = True         # (a FeatureView: the scorer it wraps)
    if args.metric == GRAM_METRIC and world > 1:
        raise SystemExit("--metric gram is single-GPU for now: run it with --ngpu 1")
    layer = args.target_layer if isinstance(args.target_layer, list) else [args.target_layer]
    taps = cli_taps(args, scorer) if args.taps else None
    if rank == 0:
        print(f"=========seed {args.seed}=========")
        if taps is None:
            print(f"Experiment on {args.target_block}, layer {args.target_layer}, timestep {args.target_step}:")
    if args.dataset == "retrieval":
        rc = run_retrieval(args, scorer, layer)
        _resize_report(args, rank)
        return rc
    if args.dataset == "nights":
        rows = H.read_nights_csv(args.image_path)
        trip = [(r["ref"], r["left"], r["right"], r["prompt"]) for r in rows]
    elif args.dataset == "sref":
        trip = sref_triplets(args.image_path, args.seed, args.prompt, args.experiments)
    else:
        trip = cute_triplets(args.image_path, args.seed)
    if args.dataset != "nights":
        rows = None
    if taps is not None:
        # one forward per image batch serves every tap; then one section per tap, as a one-tap run prints it after its banner
        from .sweep import score_path_triplets_taps, tap_label
        if args.selftest_shard:
            s_ab, s_ac, bad = _selftest_scores_taps(trip, rank, world, len(taps))
        else:
            s_ab, s_ac, bad = score_path_triplets_taps(scorer, trip, args.image_size, taps, args.target_step, args.seed,
                                                       args.similarity, rank, world, args.batch, args.unet_batch,
                                                       return_status=True)
        if rank == 0:
            for t, tap in enumerate(taps):
                block, tl = tap_label(tap)
                block = args.target_block if isinstance(tap, int) else block      # (a DiT run prints the ignored block flag)
                print(f"Experiment on {block}, layer {tl}, timestep {args.target_step}:")
                _report(args, trip, rows, s_ab[t], s_ac[t], bad[t])
    else:
        masks = None
        if args.mask_path is not None:
            from .regions import triplet_mask_paths
            masks, missing = triplet_mask_paths(trip, args.image_path, args.mask_path)
            if rank == 0:
                print(f"Region scores: masks from {args.mask_path}; {missing} image(s) without a mask file are scored whole")
                if args.soft_masks:
                    print("Soft regions: a mask's area average on the token grid is the token's weight")
        exemplar = None
        if args.transfer_masks and masks is not None:
            no_ref = len({t[0] for t, mk in zip(trip, masks) if mk[0] is None})
            masks = [mk[0] for mk in masks]
            if not args.selftest_shard:
                from .transfer import ExemplarGuide
                exemplar = ExemplarGuide(args.transfer_threshold, args.soft_masks)
            if rank == 0:
                print(f"Exemplar-guided regions: only the reference images read their masks, threshold {args.transfer_threshold:g} x the "
                      f"mean attention mass; {no_ref} reference image(s) without a mask file make their candidates whole")
        guide = None
        if args.text_attn is not None and not args.selftest_shard:
            from .textattn import TextGuide
            guide = TextGuide(args.text_attn, args.text_threshold, **({"soft": True} if args.text_soft else {}))
            if rank == 0:
                print(f"Text-guided regions: {'the words ' + ' '.join(args.text_attn) if args.text_attn else 'every content token'} "
                      f"of each prompt, threshold {args.text_threshold:g} x the mean saliency")
        if args.selftest_shard:
            s_ab, s_ac, bad = _selftest_scores(trip, rank, world)
        elif args.metric == GRAM_METRIC:
            s_ab, s_ac, bad = scorer.score_path_triplets(trip, args.image_size, args.gram_full)
        else:
            s_ab, s_ac, bad = H.score_path_triplets(scorer, trip, args.image_size, args.target_block, layer, args.target_step,
                                                    args.seed, args.similarity, rank, world, args.batch, args.unet_batch,
                                                    *(() if masks is None else (masks,)), **({} if guide is None else {"text": guide}),
                                                    **({"soft": True} if args.soft_masks else {}),
                                                    **({} if exemplar is None else {"exemplar": exemplar}))
        if rank == 0:
            if exemplar is not None:
                print(f"Mean {'token weight' if args.soft_masks else 'share of tokens on'}: {exemplar.on_fraction * 100:.2f}%")
            if guide is not None:
                if args.text_soft:
                    print(f"Mean token weight: {guide.on_fraction * 100:.2f}%")
                else:
                    print(f"Mean share of tokens on: {guide.on_fraction * 100:.2f}%")
            _report(args, trip, rows, s_ab, s_ac, bad)
    _resize_report(args, rank)
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()
    return 0


def run_retrieval(args, scorer, layer) -> int:
    """--dataset retrieval: the query x gallery score matrix (retrieval.score_path_matrix) and one ranking file per query."""
    from . import retrieval as R
    from .inputs import path_latents
    queries, gallery = R.list_images(args.query_path), R.list_images(args.image_path)
    try:
        R.ranking_names(queries, args.query_path)               # two queries that would share a ranking file: refused before scoring
    except ValueError as e:
        raise SystemExit(str(e))
    exemplar = regions = None
    if args.metric == GRAM_METRIC:
        m, bad = scorer.score_path_matrix(queries, gallery, args.image_size, getattr(args, "gram_full", False), return_status=True)
    elif getattr(args, "transfer_masks", False):         # (a plain Namespace without the flag: off)
        from .regions import mask_path_for
        from .transfer import ExemplarGuide
        exemplar = ExemplarGuide(args.transfer_threshold, args.soft_masks)
        qmasks = [mask_path_for(p, args.query_path, args.query_mask_path) for p in queries]
        print(f"Exemplar-guided retrieval: only the queries read their masks (from {args.query_mask_path}), threshold "
              f"{args.transfer_threshold:g} x the mean attention mass; {sum(1 for f in qmasks if f is None)} query image(s) without a "
              "mask file make their gallery images whole")
        res = R.score_path_matrix(scorer, queries, gallery, args.image_size, args.prompt, args.target_block, layer, args.target_step,
                                  args.seed, args.similarity, return_status=True, masks_a=qmasks, exemplar=exemplar,
                                  return_regions=bool(getattr(args, "save_transfer", False) and queries and gallery))
        (m, bad), regions = res[:2], res[2:]
        if queries and gallery:
            print(f"Mean {'token weight' if args.soft_masks else 'share of tokens on'}: {exemplar.on_fraction * 100:.2f}%")
    elif args.query_mask_path is not None or args.gallery_mask_path is not None:
        from .regions import mask_path_for
        masks, missing = {}, 0
        for side, paths, root, mdir in (("masks_a", queries, args.query_path, args.query_mask_path),
                                        ("masks_b", gallery, args.image_path, args.gallery_mask_path)):
            if mdir is not None:
                masks[side] = [mask_path_for(p, root, mdir) for p in paths]
                missing += sum(1 for f in masks[side] if f is None)
        print(f"{'Soft' if args.soft_masks else 'Region'} score matrix: masks from "
              f"{' and '.join(d for d in (args.query_mask_path, args.gallery_mask_path) if d)}; "
              f"{missing} image(s) without a mask file are scored whole")
        if args.soft_masks:
            masks["soft"] = True
        if (args.save_region_maps or args.save_region_matches or args.soft_masks) and queries and gallery:
            # the matrix's own latents and draws, kept for the region maps / alignments of each query's top-k cells
            (latA,), nA, _ = path_latents(scorer, [(p,) for p in queries], (0,), args.image_size, args.seed, R.ENCODE_CHUNK)
            (latB,), _, nB = path_latents(scorer, [(p,) for p in gallery], (1,), args.image_size, args.seed, R.ENCODE_CHUNK)
            if args.soft_masks:
                from .regions import tap_grid
                grid = tap_grid(scorer, scorer.tap_of(args.target_block, layer), latA.shape[-1])
                for side, n, name in (("masks_a", len(queries), "query"), ("masks_b", len(gallery), "gallery")):
                    if side in masks:
                        masks[side] = R.set_weights(masks[side], n, grid, "cpu", side).view(n, *grid)      # (the files are read once)
                        print(f"Mean {name} token weight: {masks[side].double().mean().item() / 2.55:.2f}%")
            m, bad = R.score_latent_matrix(scorer, latA, latB, nA, nB, args.prompt, args.target_block, layer, args.target_step,
                                           args.similarity, return_status=True, **masks)
        else:
            m, bad = R.score_path_matrix(scorer, queries, gallery, args.image_size, args.prompt, args.target_block, layer,
                                         args.target_step, args.seed, args.similarity, return_status=True, **masks)
    elif not (args.save_maps or args.save_matches):
        m, bad = R.score_path_matrix(scorer, queries, gallery, args.image_size, args.prompt, args.target_block, layer,
                                     args.target_step, args.seed, args.similarity, return_status=True)
    elif queries and gallery:
        # the matrix's own latents and draws, kept for the maps / alignments of each query's top-k cells
        (latA,), nA, _ = path_latents(scorer, [(p,) for p in queries], (0,), args.image_size, args.seed, R.ENCODE_CHUNK)
        (latB,), _, nB = path_latents(scorer, [(p,) for p in gallery], (1,), args.image_size, args.seed, R.ENCODE_CHUNK)
        m, bad = R.score_latent_matrix(scorer, latA, latB, nA, nB, args.prompt, args.target_block, layer, args.target_step,
                                       args.similarity, return_status=True)
    else:
        m, bad = R.score_path_matrix(scorer, queries, gallery, args.image_size, args.prompt, args.target_block, layer,
                                     args.target_step, args.seed, args.similarity, return_status=True)
    files = R.write_rankings(args.out_path, queries, gallery, m, args.topk, args.similarity, args.query_path)
    if bad:
        print(f"WARNING: {bad} score(s) are NaN/inf (ranked last)")
    print(f"Score matrix {tuple(m.shape)} ({len(queries)} queries x {len(gallery)} gallery images, {args.similarity}); "
          f"top-{min(args.topk, len(gallery))} rankings of {len(files)} queries written to {args.out_path}")
    if regions:
        import numpy as np
        _vals, idx = R.topk(m, args.topk, args.similarity)
        region, mass = (t.cpu() for t in regions)
        for i, fn in enumerate(files):
            np.savez(os.path.splitext(fn)[0] + ".transfer.npz", gallery=np.array([gallery[j] for j in idx[i].tolist()]),
                     region=region[i, idx[i]].numpy(), mass=mass[i, idx[i]].numpy())
        print(f"Transferred regions {region.shape[2]}x{region.shape[3]} of the top-{idx.shape[1]} cells of {len(files)} queries written "
              f"to {args.out_path}")
    if args.save_maps and queries and gallery:
        from . import maps as M
        _vals, idx = R.topk(m, args.topk, args.similarity)
        k = idx.shape[1]
        mp = M.score_latent_pair_maps(scorer, latA.repeat_interleave(k, 0), latB[idx.reshape(-1).to(latB.device)], nA, nB,
                                      args.prompt, args.target_block, layer, args.target_step, args.similarity)
        mfiles = M.write_map_files(args.out_path, queries, gallery, idx, mp, args.query_path)
        print(f"Similarity maps {mp.grid[0]}x{mp.grid[1]} of the top-{k} cells of {len(mfiles)} queries written to {args.out_path}")
    if args.save_matches and queries and gallery:
        from . import align as A
        _vals, idx = R.topk(m, args.topk, args.similarity)
        k = idx.shape[1]
        al = A.score_latent_pair_alignment(scorer, latA.repeat_interleave(k, 0), latB[idx.reshape(-1).to(latB.device)], nA, nB,
                                           args.prompt, args.target_block, layer, args.target_step)
        afiles = A.write_match_files(args.out_path, queries, gallery, idx, al, args.query_path)
        print(f"Token alignments {al.grid[0]}x{al.grid[1]} of the top-{k} cells of {len(afiles)} queries written to {args.out_path}")
    if (args.save_region_maps or args.save_region_matches) and queries and gallery:
        from .regions import kind_of, tap_grid
        _vals, idx = R.topk(m, args.topk, args.similarity)
        k = idx.shape[1]
        cells = idx.reshape(-1)
        # the matrix's own token masks or weights (a missing or empty mask: the whole image), one pair of them per top-k cell
        grid = tap_grid(scorer, scorer.tap_of(args.target_block, layer), latA.shape[-1])
        set_of = kind_of(args.soft_masks).set_rows
        soft = {"soft": True} if args.soft_masks else {}
        mA = set_of(masks.get("masks_a"), len(queries), grid, "cpu", "masks_a").repeat_interleave(k, 0)
        mB = set_of(masks.get("masks_b"), len(gallery), grid, "cpu", "masks_b")[cells.cpu()]
        if args.save_region_maps:
            from . import maps as M
            mp = M.score_latent_pair_maps(scorer, latA.repeat_interleave(k, 0), latB[cells.to(latB.device)], nA, nB, args.prompt,
                                          args.target_block, layer, args.target_step, args.similarity, maskA=mA, maskB=mB, **soft)
            mfiles = M.write_map_files(args.out_path, queries, gallery, idx, mp, args.query_path)
            print(f"{'Soft region' if args.soft_masks else 'Region'} maps {mp.grid[0]}x{mp.grid[1]} of the top-{k} cells of {len(mfiles)} queries written to {args.out_path}")
        if args.save_region_matches:
            from . import align as A
            al = A.score_latent_pair_alignment(scorer, latA.repeat_interleave(k, 0), latB[cells.to(latB.device)], nA, nB, args.prompt,
                                               args.target_block, layer, args.target_step, maskA=mA, maskB=mB, **soft)
            afiles = A.write_match_files(args.out_path, queries, gallery, idx, al, args.query_path)
            print(f"{'Soft region' if args.soft_masks else 'Region'} alignments {al.grid[0]}x{al.grid[1]} of the top-{k} cells of {len(afiles)} queries written to {args.out_path}")
    return 0


def main(argv=None) -> int:
    argv = list(sys.argv[1:] if argv is None else argv)
    args = arg_parse(argv)
    if "WORLD_SIZE" in os.environ:
        # --ngpu counts the GPUs of THIS node: under a launcher that is LOCAL_WORLD_SIZE (WORLD_SIZE on one node).  A launch
        # that left --ngpu at its default adopts the launcher's count; an explicit, different --ngpu is refused as mislabelled.
        local_world = int(os.environ.get("LOCAL_WORLD_SIZE", os.environ["WORLD_SIZE"]))
        explicit = args.ngpu is not None            # (default None: every spelling argparse accepts counts as given)
        if not explicit:
            if local_world != 1:
                print(f"diffsim_amd: --ngpu not given; using the launcher's {local_world} rank(s) on this node", file=sys.stderr)
            args.ngpu = local_world
        elif local_world != args.ngpu:
            raise SystemExit(f"--ngpu {args.ngpu} but the launcher started {local_world} rank(s) on this node "
                             f"(LOCAL_WORLD_SIZE / WORLD_SIZE): refusing to run a mislabelled launch")
    if args.ngpu is None:
        args.ngpu = 1
    if args.dataset == "retrieval":
        if args.ngpu > 1:
            raise SystemExit("--dataset retrieval is single-GPU for now: run it with --ngpu 1")
        if args.selftest_shard:
            raise SystemExit("--selftest_shard checks the triplet sharding; --dataset retrieval has none")
        if not args.query_path or not args.image_path or not args.out_path:
            raise SystemExit("--dataset retrieval needs --query_path, --image_path (the gallery) and --out_path")
    if args.ngpu > 1 and "WORLD_SIZE" not in os.environ:
        from .parallel import spawn_ranks              # the parent never touches the GPU
        return spawn_ranks(args.ngpu, [sys.executable, "-m", "diffsim_amd"] + argv)
    return run(args)
