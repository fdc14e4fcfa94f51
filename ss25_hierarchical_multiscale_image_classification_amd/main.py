"""Command line mirroring the hot-path flags of the reference's ``src/main.py``
(:1073-1166): ``--patch``, ``--patch_level {0,1,2,3,all}``, ``--extract_features``,
``--train``, ``--train_strategy``, ``--strategy {balanced,weighted_loss,self_supervised}``.

Layout under ``--data_root`` (default ``./data/camelyon16``, README.md:142-164):
    train/img/<slide>.{npz,tif}      slides   (.tif: tiled pyramidal TIFF / BigTIFF, levels 0-3 are used;
                                              .npz: keys level0..levelN uint8[H,W,3])
    train/mask/annotations/<slide>.xml
    patches/level_L/<slide>/...      extractor output
Outputs of ``--extract_features`` are written to the current directory exactly like
the reference (patch_features_L.npy, patch_labels_L.npy, patch_paths_L.txt).

Additive flags: ``--data_root``, ``--synthetic W,H,SEED[,NAME]`` (repeatable; a slide
made on the GPU instead of a file), ``--write_png`` (also emit the reference's PNG
tree), ``--precision {bf16,fp16,fp16x3,fp16q8,fp32}``, ``--weights PATH``, ``--stride N``,
``--world_size N`` (one process per GPU over RCCL where the reference wraps its model in
nn.DataParallel, src/main.py:481-482, :841-842: ``--patch`` / ``--extract_features`` shard the
slides, ``--train*`` the batches; started by this program itself before it touches a GPU).

``--detect`` writes those detection lists (``detect.py``): every slide in ``<data_root>/test/img`` (and every
``--synthetic`` spec) is scanned densely with the two-class network of ``--weights`` at the levels of ``--patch_level``
(``all`` = levels 0-3 fused cell by cell), and the tumour probability map, its Gaussian smoothing and the non-maximum
suppression run on the device; one ``probability,x,y`` line per detection goes to
``./models/first_model/model_predictions_csv/<case>.csv`` (``--detect_save_maps``: the fused map to
``./models/first_model/heatmaps/<case>.npy``).  ``--detect_cell`` / ``--detect_fuse`` / ``--detect_sigma`` /
``--detect_radius`` / ``--detect_threshold`` / ``--detect_max`` set the post-processing; under ``--world_size N`` the slides
are sharded.  ``--detect --run_evaluation`` detects first, then scores.  ``--detect_tta {none,rot4,d4}`` (``tta.py``) scores every
window in 1, 4 or 8 views of the square -- the rotations by 90 degrees, with ``d4`` each also mirrored -- made on the device from
the patch buffer, and averages the tumour probabilities: about as many scans as views.  The slide's line then ends with
``, V views`` and ``--detect_save_maps`` also writes ``heatmaps/<case>_tta_range.npy``, the map of the per-window range over the
views.  Default ``none``: no byte written or printed changes.

``--tissue_filter otsu`` replaces the whiteness test (``mean > 240``, the reference's rule and the default ``white``) with an
Otsu tissue mask made on the device (``tissue.py``): a saturation threshold on a 1 : 32 thumbnail of the coarsest level, a 3 x 3
opening, a dilation by ``--tissue_dilate`` mask pixels, never below ``--tissue_sat_floor``; a window is kept when at least
``--tissue_min`` of its mask rectangle is tissue.  Honoured by ``--patch``, ``--extract_features`` on the fused slide route and
``--detect``; ``--tissue_save_masks`` writes ``./models/first_model/tissue_masks/<case>.npy`` (uint8[mh][mw]).

``--stain_norm macenko`` normalises every slide's H&E colours on the device right after it is opened (``stain.py``): Macenko's
stain vectors are fitted on the coarsest level (tissue pixels: optical density of every channel at least ``--stain_beta``, and inside
the Otsu mask under ``--tissue_filter otsu``; the extreme angles at the ``--stain_alpha`` / 100 - ``--stain_alpha`` percentiles) and
every level is mapped in place to the usual Macenko target, or to the ``HE`` / ``maxC`` of ``--stain_target FILE.json``;
``--stain_save_fit`` writes ``./models/first_model/stain/<case>.json``.  Honoured by ``--patch``, ``--extract_features`` on the fused
slide route and ``--detect``.  The Otsu mask is made from the original pixels and is not recomputed; the ``white`` rule
(``mean > 240``) sees the normalised pixels.  Default ``none``: no byte of any output changes.

``--aug_hed SIGMA`` is the training side of the same problem (``augment_hed.py``): under ``--device_aug`` / ``--from_slides`` every
training view of ``--train`` / ``--train_strategy`` (both SimCLR views of ``self_supervised`` too; normal and tumour patches alike)
gets a random HED stain map of its own in optical-density space, alpha ~ U(1 - SIGMA, 1 + SIGMA) and beta ~ U(-SIGMA, SIGMA) per
stain, inside the colour kernel.  Keyed by ``--seed``; validation is never augmented; refused without the device pipeline.
Default 0: no byte of any output and no call path changes.

``--png_encoder device`` moves the PNG encoding of ``--patch --write_png`` to the device (``png_encode.py``,
``include/hipac_png.h``): the row filter (the cheapest of the five types per row), deflate (distance-1 run matches and one stored,
fixed or dynamic Huffman block per band of at most 24 KiB of filtered rows, whichever is smallest) and both checksums run in HBM
for batches of windows, one copy per batch brings the compressed bytes back and the host only writes the files.  The same file
names, the same pixels after decoding, the same skipping of files that exist; the bytes of the files differ from Pillow's (run
matches only, one IDAT chunk per band, the project's own Huffman builder).  Refused without ``--write_png``.  Default ``host``: no
byte written or printed changes.

``--run_evaluation`` scores ``./models/first_model/model_predictions_csv/*.csv`` (written by ``--detect``, or by
``features.save_froc_csv`` with one line per window) against ``<data_root>/test/mask`` with the CAMELYON16 FROC script's rules, the
evaluation masks made on the device (``froc.py``); it writes ``froc_results.json`` (and ``froc.png``).
``--eval_roc`` adds the slide-level ROC and AUC of the same cases (``roc_results.json``, ``roc.png``; scores from the CSVs or
from ``--eval_slide_scores FILE``), ``--eval_bootstrap B`` the ``--eval_ci`` percent percentile-bootstrap intervals of the
score, its six sensitivities and the AUC over B resamples of the cases, drawn and scanned on the device and keyed by
``--seed`` (``froc_ci.py`` -> ``bootstrap_results.json``).  Without them every byte stays as it was.

``--train_mil`` trains the ABMIL slide classifier (``mil_train.py``, the loop of the reference's
``experiments/experiment_configs.yaml``) on the ``patch_features_L.npy`` / ``patch_labels_L.npy`` / ``patch_paths_L.txt``
triple of ``--patch_level L`` in the working directory and writes ``models/mil_model.pth`` and ``results/metrics.json``;
``--predict_mil`` scores every bag of the triple with ``--mil_model`` into ``results/mil_predictions.csv``.
``--mil_heads K`` (1..8, the yaml's ``attention_heads: 8``) trains multi-head attention pooling (``mil_heads.py``): K
softmaxes over one shared hidden layer, the K pooled vectors concatenated; ``--predict_mil`` reads K from the saved model.
``--mil_save_attention`` makes ``--predict_mil`` also write ``results/mil_attention.npy``, float32 [patches, K] in the
order of ``patch_paths_L.txt``.
``--mil_gated`` trains the gated attention of Ilse et al. 2018 (``mil_gated.py``): a learned sigmoid gate ``aggregator.attn_G``
over the hidden units, for any ``--mil_heads``; ``--predict_mil`` reads gatedness from the saved model and takes no flag.
``--mil_levels 1,2,3`` trains the multiscale model (``mil_levels.py``): a slide's bag holds the rows of the triples of all the
named levels, every level has its own attention branch and softmax, the pooled vectors are concatenated; ``--patch_level`` is
then not read.  ``--predict_mil`` reads the levels from the saved model; ``--mil_save_attention`` writes one
``results/mil_attention_<L>.npy`` per level.

``--validate`` is the reference's feature sanity check (src/main.py:1017-1070) on the device: a two-component PCA and a
class-weighted logistic-regression probe (Newton's method) on ``patch_features_<L>.npy`` / ``patch_labels_<L>.npy`` of
``--patch_level`` -> ``results/validate_<L>.json``; ``--validate_save_pca`` adds ``results/pca_<L>.npy``.  No t-SNE.
``--validate_knn K`` adds the weighted k-nearest-neighbour probe (knn.py); ``--validate_save_knn`` its neighbour table.

``--eval_patches`` is the reference's ``--evaluate`` stage (src/main.py:974-1015) under a new name (``--evaluate`` itself
stays out of scope): the checkpoint of ``--weights`` (default ``src/models/resnet18_patch_classifier.pth``, where ``--train``
saves) is scored on the validation set of ``--train`` -- the PNG tree of ``--patch_level``, its device pool under
``--device_aug``, or the slides under ``--from_slides`` -- and ``evaluate.py`` writes ``results/evaluate_<L>.json``: confusion
matrix, the quantities of the reference's ``src/utils/metrics.py``, a ROC / AUC and average precision over 4096 probability
bins, and a per-slide table, all tallied on the device in integers.  ``--eval_threshold T`` decides by ``p > T`` instead of the
argmax, ``--eval_unbalanced`` scores every patch of the validation slides, ``--eval_bootstrap B`` / ``--eval_ci`` / ``--seed``
add percentile intervals from B resamples of the validation slides.

Everything else outside the hot path (download, plots) is out of scope and the
corresponding reference flags are accepted but answered with a clear message.
"""
from __future__ import annotations

import argparse
import os
import sys
from typing import List, Optional

import numpy as np
import torch

OUT_OF_SCOPE = ("download", "remote", "prepare", "validation", "evaluate",
                "balance_dataset", "count_tumor_patches", "patch_one_slide", "slide", "move_files",
                "check_good_downloaded_files")


def _eval_bootstrap(text: str) -> int:
    v = int(text)
    if not 0 <= v <= 65536:
        raise argparse.ArgumentTypeError(f"takes 0 (off) .. 65536 replicates, got {v}")
    return v


def _eval_ci(text: str) -> float:
    v = float(text)
    if not 0.0 < v < 100.0:
        raise argparse.ArgumentTypeError(f"takes a percentage above 0 and below 100, got {text}")
    return v


def _eval_threshold(text: str) -> float:
    v = float(text)
    if not 0.0 < v < 1.0:
        raise argparse.ArgumentTypeError(f"takes a probability strictly between 0 and 1, got {text}")
    return v


def check_eval_patches_args(parser, args):
    """--eval_threshold / --eval_unbalanced without --eval_patches are argparse errors (exit status 2): a flag that is dropped
    silently would be worse than none."""
    if not args.eval_patches:
        if args.eval_threshold is not None:
            parser.error(f"--eval_threshold {args.eval_threshold:g} is an option of --eval_patches")
        if args.eval_unbalanced:
            parser.error("--eval_unbalanced is an option of --eval_patches")


def _aug_hed(text: str) -> float:
    from .augment_hed import check_sigma

    try:
        return check_sigma(float(text))
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e)) from None


def check_aug_args(parser, args):
    """--aug_hed without the device input pipeline is refused as an argparse error (exit status 2): the host transforms have no
    HED stage, and a flag that is dropped silently would be worse than none."""
    if args.aug_hed > 0.0:
        if not (args.train or args.train_strategy):
            parser.error(f"--aug_hed {args.aug_hed:g} is an option of --train / --train_strategy")
        if not (args.device_aug or args.from_slides):
            parser.error(f"--aug_hed {args.aug_hed:g} needs the device input pipeline: give --device_aug or --from_slides")


def check_png_args(parser, args):
    """--png_encoder device without --write_png is refused as an argparse error (exit status 2): there would be nothing to
    encode, and a flag that is dropped silently would be worse than none."""
    if args.png_encoder != "host" and not args.write_png:
        parser.error(f"--png_encoder {args.png_encoder} is an option of --patch --write_png")


def check_tta_args(parser, args):
    """--detect_tta without --detect is refused as an argparse error (exit status 2): the views are an option of the detector
    alone, and a flag that is dropped silently would be worse than none."""
    if args.detect_tta != "none" and not args.detect:
        parser.error(f"--detect_tta {args.detect_tta} is an option of --detect")


def _validate_knn(text: str) -> int:
    v = int(text)
    if not 1 <= v <= 256:
        raise argparse.ArgumentTypeError(f"takes a neighbour count in 1..256, got {text}")
    return v


def _validate_knn_T(text: str) -> float:
    v = float(text)
    if not 0.01 <= v <= 10.0:
        raise argparse.ArgumentTypeError(f"takes a temperature in 0.01..10, got {text}")
    return v


def check_validate_knn_args(parser, args):
    """--validate_knn / --validate_knn_T / --validate_save_knn without --validate, and the latter two without --validate_knn,
    are refused as argparse errors (exit status 2): a flag that is dropped silently would be worse than none."""
    given = [name for name, on in (("--validate_knn", args.validate_knn is not None), ("--validate_knn_T", args.validate_knn_T is not None),
                                   ("--validate_save_knn", args.validate_save_knn)) if on]
    if given and not args.validate:
        parser.error(f"{given[0]} is an option of --validate")
    if args.validate_knn is None and given:
        parser.error(f"{given[0]} needs --validate_knn K")


def tta_views(args):
    """The views of --detect_tta as ``detect_slide`` and ``score_slide`` number them (``tta.MODES``)."""
    from . import tta

    return tta.MODES[args.detect_tta]


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="HiPAC hot path on MI355X (patch extraction + ResNet18 scoring)")
    # --- the reference's surface (src/main.py:1075-1093) ---
    p.add_argument("-p", "--patch", action="store_true", help="Extract patches")
    p.add_argument("--patch_level", type=str, default="3", help="WSI level (0, 1, 2, 3, or 'all')")
    p.add_argument("--extract_features", action="store_true", help="Extract features from patches")
    p.add_argument("-train", "--train", action="store_true", help="Train ResNet18 patch classifier")
    p.add_argument("--train_strategy", action="store_true", help="Train with a specific strategy")
    p.add_argument("--strategy", type=str, default="self_supervised",
                   choices=["balanced", "weighted_loss", "self_supervised"])
    p.add_argument("--run_evaluation", action="store_true",
                   help="CAMELYON16 FROC evaluation of the detection CSVs (src/main.py:1168-1225)")
    p.add_argument("--eval_roc", action="store_true",
                   help="--run_evaluation: also the slide-level ROC and its AUC over the evaluated cases -> roc_results.json (and "
                        "roc.png); a case's score is its largest detection probability")
    p.add_argument("--eval_slide_scores", type=str, default=None, metavar="FILE",
                   help="--eval_roc: take the scores from FILE, lines 'case,score[,...]' (results/mil_predictions.csv fits)")
    p.add_argument("--eval_bootstrap", type=_eval_bootstrap, default=0, metavar="B",
                   help="--run_evaluation: percentile-bootstrap intervals of the score, the six sensitivities (and the AUC) over B "
                        "resamples of the cases, drawn on the device and keyed by --seed -> bootstrap_results.json (0 = off, at most 65536)")
    p.add_argument("--eval_ci", type=_eval_ci, default=95.0, metavar="PCT", help="--eval_bootstrap: the interval in percent (above 0, below 100)")
    p.add_argument("--eval_patches", action="store_true",
                   help="the reference's --evaluate stage (src/main.py:974-1015): score the checkpoint of --weights (default "
                        "src/models/resnet18_patch_classifier.pth) on the validation patches of --train, tallied on the device -> "
                        "results/evaluate_<L>.json; --eval_bootstrap / --eval_ci / --seed add intervals over resamples of the slides")
    p.add_argument("--eval_threshold", type=_eval_threshold, default=None, metavar="T",
                   help="--eval_patches: a patch is called tumour when its probability is > T (strictly between 0 and 1; default: "
                        "the network's argmax)")
    p.add_argument("--eval_unbalanced", action="store_true",
                   help="--eval_patches: score every patch of the validation slides instead of the class-balanced set of --train")
    p.add_argument("--validate", action="store_true",
                   help="sanity check of the feature files of --patch_level in the working directory (src/main.py:1017-1070): "
                        "PCA and a logistic-regression probe on the device -> results/validate_<L>.json (rank 0)")
    for name in OUT_OF_SCOPE:
        if name in ("patch_one_slide", "slide"):
            p.add_argument(f"--{name}", type=str, default=None, help="(reference flag; out of scope here)")
        else:
            p.add_argument(f"--{name}", action="store_true", help="(reference flag; out of scope here)")
    # --- additive ---
    p.add_argument("--data_root", type=str, default=None)
    p.add_argument("--synthetic", action="append", default=[], metavar="W,H,SEED[,NAME]")
    p.add_argument("--write_png", action="store_true")
    p.add_argument("--png_encoder", choices=["host", "device"], default="host",
                   help="--patch --write_png: who encodes the patch PNGs; host = Pillow on the host, one window at a time; device = "
                        "filter, deflate and checksums on the device (png_encode.py), only compressed bytes are copied back")
    p.add_argument("--precision", choices=["bf16", "fp16", "fp16x3", "fp16q8", "fp32"], default="bf16",
                   help="MFMA operand type; fp16x3 = parity mode (fp16 pairs, three products per term: the reference's fp32 "
                        "results to 1e-3 at ~1/3 of the bf16 throughput); fp16q8 = the faster parity mode (the same pairs, cross "
                        "products on the e4m3 MX MFMA: logits within ~1e-5); fp32 = debugging reference (exact f32 MFMA, ~1/9)")
    p.add_argument("--weights", type=str, default=None, help="state_dict (.pth, any reference key layout)")
    p.add_argument("--stride", type=int, default=None, help="window stride (default: the reference's 224)")
    p.add_argument("--epochs", type=int, default=None)
    p.add_argument("--simclr_epochs", type=int, default=200, help="pre-training epochs of --strategy self_supervised (:557)")
    p.add_argument("--simclr_encoder", type=str, default=None,
                   help="--extract_features with a SimCLR encoder checkpoint (extract_features_with_simclr, src/main.py:897-932)")
    p.add_argument("--batch_size", type=int, default=512)  # BATCH_SIZE, src/main.py:46
    p.add_argument("--world_size", type=int, default=1,
                   help="number of GPUs = processes (the reference uses every visible GPU through nn.DataParallel)")
    p.add_argument("--dist_backend", default="nccl", help="process-group backend of --world_size > 1 (nccl = RCCL)")
    p.add_argument("--one_device", action="store_true",
                   help="rehearsal only: every rank uses cuda:0 (needs --dist_backend gloo; RCCL wants one GPU per rank)")
    p.add_argument("--rank_timeout", type=float, default=None, help="--world_size > 1: give up after this many seconds")
    p.add_argument("--seed", type=int, default=None, help="seed of the host-side random draws (dataset shuffles, model init); "
                                                       "with --world_size > 1 every rank uses the same one (default 0 there)")
    p.add_argument("--max_steps", type=int, default=None, help="bound the training loops (tests)")
    p.add_argument("--train_precision", choices=["fp16", "fp32"], default="fp16",
                   help="arithmetic of the classifier training step: fp16 = the reference's autocast + GradScaler "
                        "(src/main.py:499-508), fp32 = exact f32 MFMA")
    p.add_argument("--device_aug", action="store_true",
                   help="training loops: keep the decoded patches in HBM and make every batch's augmented views on the device "
                        "(hipac_augment_views; classifier loops: 224-pixel patches) instead of in DataLoader workers")
    p.add_argument("--from_slides", action="store_true",
                   help="--train / --train_strategy: no PNG tree -- the kept windows go from the slides in HBM straight into the "
                        "training pool (implies the device input pipeline)")
    p.add_argument("--aug_hed", type=_aug_hed, default=0.0, metavar="SIGMA",
                   help="training loops with --device_aug / --from_slides: HED stain augmentation of every training view on the "
                        "device, alpha ~ U(1 - SIGMA, 1 + SIGMA) and beta ~ U(-SIGMA, SIGMA) per stain (0 = off, at most 0.5; "
                        "0.05 light, 0.2 strong); the draws are keyed by --seed")
    p.add_argument("--simclr_precision", choices=["fp16", "fp32"], default="fp32",
                   help="arithmetic of the SimCLR pre-training step (the reference's loop is fp32, src/models/simclr.py:85-96)")
    p.add_argument("--train_mil", action="store_true",
                   help="train the MIL slide classifier on the feature triple of --patch_level in the working directory "
                        "(under --world_size N rank 0 trains: the step is small and is not sharded)")
    p.add_argument("--predict_mil", action="store_true",
                   help="score every bag of the feature triple with --mil_model -> results/mil_predictions.csv (rank 0)")
    p.add_argument("--mil_pooling", choices=["attention", "mean", "max"], default="attention")
    p.add_argument("--mil_by_slide", action="store_true", help="one bag per slide (default: the reference's key, one per slide column)")
    p.add_argument("--mil_epochs", type=int, default=50)
    p.add_argument("--mil_bag_size", type=int, default=None, help="sample at most this many patches per bag and epoch (default: the whole bag)")
    p.add_argument("--mil_bags_per_step", type=int, default=32)
    p.add_argument("--mil_model", type=str, default=os.path.join("models", "mil_model.pth"))
    p.add_argument("--mil_dropout", type=float, default=0.0, metavar="P",
                   help="dropout probability of the MIL head: on the feature rows and the classifier's hidden layer during --train_mil, "
                        "and of the Monte-Carlo samples of --predict_mil (the reference's yaml: 0.5; default 0 = none); seeded by --seed")
    p.add_argument("--mil_mc_samples", type=int, default=0, metavar="T",
                   help="--predict_mil: also run T Monte-Carlo dropout forwards per bag -> results/mil_uncertainty.csv "
                        "(the reference's yaml: 100; needs --mil_dropout > 0)")
    p.add_argument("--mil_heads", type=int, default=None, metavar="K",
                   help="attention heads of the MIL head, 1..8 (the reference's yaml: 8; default 1): K softmaxes over one shared "
                        "hidden layer, the K pooled vectors concatenated in front of the classifier.  Attention pooling only, and "
                        "not with --mil_dropout / --mil_mc_samples.  --predict_mil reads K from the model; if given it must agree")
    p.add_argument("--mil_gated", action="store_true",
                   help="--train_mil: gated attention (Ilse et al. 2018, eq. 9; CLAM's form): the score of a patch is "
                        "U (tanh(V x) * sigmoid(G x)), with two more state_dict keys aggregator.attn_G.*.  Attention pooling only, "
                        "any --mil_heads, not with --mil_dropout / --mil_mc_samples.  --predict_mil reads it from the model")
    p.add_argument("--mil_levels", type=str, default=None, metavar="L,L,...",
                   help="--train_mil over several pyramid levels: two to four distinct levels out of 0..3, ascending, such as 1,2,3. "
                        "A slide's bag holds the rows of all of them, every level has its own attention branch and softmax; "
                        "--patch_level is ignored.  Attention pooling only, not with --mil_heads > 1, --mil_gated, --mil_dropout / "
                        "--mil_mc_samples.  --predict_mil reads the levels from the model; if given they must agree")
    p.add_argument("--mil_save_attention", action="store_true",
                   help="--predict_mil with attention pooling: also write results/mil_attention.npy, float32 [patches, K], row i "
                        "= the attention weights of line i of patch_paths_L.txt inside its bag")
    p.add_argument("--mil_threshold", type=float, default=0.5, help="--mil_mc_samples: prediction = mean probability > this")
    p.add_argument("--detect", action="store_true",
                   help="write the detection CSVs --run_evaluation scores: dense scan of <data_root>/test/img at the levels of "
                        "--patch_level, probability map, smoothing and NMS on the device")
    p.add_argument("--detect_cell", type=int, default=224, help="cell of the probability map in level-0 pixels (divides 1792)")
    p.add_argument("--detect_fuse", choices=["mean", "max"], default="mean", help="how the levels' maps are combined per cell")
    p.add_argument("--detect_sigma", type=float, default=1.0, help="Gaussian smoothing of the fused map, in cells (0 = none)")
    p.add_argument("--detect_radius", type=int, default=4, help="NMS radius in cells")
    p.add_argument("--detect_threshold", type=float, default=0.5, help="smallest probability of a detection")
    p.add_argument("--detect_max", type=int, default=2000, help="most detections per slide")
    p.add_argument("--detect_save_maps", action="store_true", help="also write models/first_model/heatmaps/<case>.npy (float32[gh][gw])")
    p.add_argument("--detect_tta", choices=["none", "rot4", "d4"], default="none",
                   help="--detect: average the tumour probability of every window over its 4 rotations (rot4) or its 8 rotations "
                        "and mirror images (d4), made on the device; about as many scans as views")
    p.add_argument("--tissue_filter", choices=["white", "otsu"], default="white",
                   help="which windows are kept: white = the reference's mean > 240 test, otsu = an Otsu saturation mask of the slide")
    p.add_argument("--tissue_min", type=float, default=0.05, help="otsu: smallest tissue fraction of a window's mask rectangle (0..1)")
    p.add_argument("--tissue_dilate", type=int, default=1, help="otsu: radius of the mask's final dilation in mask pixels (0..8)")
    p.add_argument("--tissue_sat_floor", type=int, default=16, help="otsu: the saturation threshold never goes below this (0..255)")
    p.add_argument("--tissue_save_masks", action="store_true", help="otsu: also write models/first_model/tissue_masks/<case>.npy (uint8[mh][mw])")
    p.add_argument("--stain_norm", choices=["none", "macenko"], default="none",
                   help="macenko: fit the slide's stain vectors on the device and map every level to the target appearance in place")
    p.add_argument("--stain_alpha", type=float, default=1.0, help="macenko: percentile of the stain angles, percent (> 0 and < 50)")
    p.add_argument("--stain_beta", type=float, default=0.15, help="macenko: smallest optical density of a tissue pixel (> 0 and <= 1)")
    p.add_argument("--stain_target", type=str, default=None, help="macenko: JSON with the HE and maxC to map to (written by --stain_save_fit)")
    p.add_argument("--stain_save_fit", action="store_true", help="macenko: also write models/first_model/stain/<case>.json (HE, maxC, n, status)")
    p.add_argument("--validate_save_pca", action="store_true",
                   help="--validate: also write results/pca_<L>.npy, float32 [N, 2], row i = the two PCA coordinates of line i of "
                        "patch_paths_<L>.txt")
    p.add_argument("--validate_knn", type=_validate_knn, default=None, metavar="K",
                   help="--validate: also the weighted k-nearest-neighbour probe (Wu et al. 2018) with K neighbours (1..256) on the "
                        "probe's split, searched on the device; absent = off")
    p.add_argument("--validate_knn_T", type=_validate_knn_T, default=None, metavar="T",
                   help="--validate_knn: the temperature of the neighbour weights exp((s - s_best) / T), 0.01..10 (default 0.07)")
    p.add_argument("--validate_save_knn", action="store_true",
                   help="--validate_knn: also write results/knn_<L>.npy, int32 [n_test, 1 + K]: a test row and its K neighbours, "
                        "nearest first, as line numbers of patch_paths_<L>.txt")
    p.add_argument("--validate_C", type=float, default=1.0, help="--validate: inverse regularisation strength of the probe (> 0)")
    p.add_argument("--validate_tol", type=float, default=1e-4, help="--validate: the probe stops at max |gradient| <= this")
    p.add_argument("--_child", action="store_true", help=argparse.SUPPRESS)
    return p


def data_root(args) -> str:
    return args.data_root or os.path.join(os.getcwd(), "data", "camelyon16")


def levels_of(args) -> List[int]:
    return [0, 1, 2, 3] if args.patch_level == "all" else [int(args.patch_level)]


def list_slides(args, split: str = "train"):
    """[(name, opener)] of every slide in processing order -- synthetic specs first, then the files in <split>/img --
    without loading any: ``opener()`` puts the slide into HBM (a rank opens only the slides it owns).  The annotations of
    <split>/mask/annotations are attached where they exist (they label the windows; detection does not read the labels)."""
    from .extract import DeviceSlide, parse_annotation_xml

    out = []
    for spec in args.synthetic:
        parts = spec.split(",")
        w, h, seed = int(parts[0]), int(parts[1]), int(parts[2])
        name = parts[3] if len(parts) > 3 else f"synthetic_{seed}"
        out.append((name, lambda w=w, h=h, seed=seed, name=name: DeviceSlide.synthetic(w, h, seed=seed, name=name)))
    img_dir = os.path.join(data_root(args), split, "img")
    if not os.path.isdir(img_dir):
        return out
    ann_dir = os.path.join(data_root(args), split, "mask", "annotations")

    def open_file(path, stem, ext):
        if ext == ".npz":
            z = np.load(path)
            levels = [torch.from_numpy(z[f"level{i}"]) for i in range(len(z.files)) if f"level{i}" in z.files]
            slide = DeviceSlide(levels, name=stem)
        else:
            # tiled pyramidal TIFF / BigTIFF (the CAMELYON16 container): own reader, openslide is not needed
            slide = DeviceSlide.from_tiff(path, name=stem)
        xml = os.path.join(ann_dir, stem + ".xml")
        if os.path.exists(xml):
            try:  # a bad annotation file costs the slide its tumour labels, not the run (src/main.py:670-675)
                slide.polygons = parse_annotation_xml(xml)
            except Exception as e:
                print(f"[WARNING] Failed to parse XML for {os.path.basename(path)}: {e}")
        return slide

    for file in sorted(os.listdir(img_dir)):
        stem, ext = os.path.splitext(file)
        if ext in (".npz", ".tif", ".tiff"):
            out.append((stem, lambda p=os.path.join(img_dir, file), stem=stem, ext=ext: open_file(p, stem, ext)))
    return out


def try_open(name: str, make):
    """The slide, or None after ``[ERROR] Could not open ...`` -- the reference opens every slide under try / except ...
    continue (src/main.py:649-653): one unreadable file costs that slide, not the run (under --world_size N: not the
    other N - 1 ranks either; the owning rank contributes zero rows for it)."""
    try:
        return make()
    except Exception as e:  # noqa: BLE001 -- whatever the reader raises for a truncated / foreign file
        print(f"[ERROR] Could not open {name}: {type(e).__name__}: {e}", flush=True)
        if int(os.environ.get("RANK", "0")) != 0:  # the launcher relays rank 0's stdout only: the other ranks report on stderr too
            print(f"[ERROR] rank {os.environ['RANK']}: could not open {name}: {type(e).__name__}: {e}", file=sys.stderr, flush=True)
        return None


def open_slides(args, rank: int = 0, world: int = 1):
    """Yield (index, DeviceSlide) of the slides this rank owns (slide i -> rank i mod world); slides that
    cannot be opened are reported and skipped."""
    from .dist import shard_units

    slides = list_slides(args)
    for i in shard_units(len(slides), rank, world):
        slide = try_open(slides[i][0], slides[i][1])
        if slide is not None:
            yield i, slide


def tissue_filter(args):
    """The ``tissue.TissueFilter`` of the --tissue_* flags, None for the default ``white``; ValueError for a bad value (no GPU
    is touched)."""
    from .tissue import TissueFilter, check_parameters

    check_parameters(args.tissue_min, args.tissue_dilate, args.tissue_sat_floor)  # checked whichever filter is chosen
    if args.tissue_filter != "otsu":
        return None
    return TissueFilter(min_frac=args.tissue_min, dilate=args.tissue_dilate, sat_floor=args.tissue_sat_floor, opening=True)


def report_tissue(args, tissue, slide):
    """The per-slide line of --tissue_filter otsu (and the mask file of --tissue_save_masks); called when the slide's results
    are back, so reading the thresholds here costs no wait inside the scan."""
    if tissue is None:
        return
    tm = tissue.mask(slide)
    print(f"[INFO] {slide.name}: {tm.report()}", flush=True)
    if args.tissue_save_masks:
        mask_dir = os.path.join(os.getcwd(), "models", "first_model", "tissue_masks")
        os.makedirs(mask_dir, exist_ok=True)
        np.save(os.path.join(mask_dir, slide.name + ".npy"), tm.mask.cpu().numpy())


def stain_norm(args):
    """The ``stain.StainNorm`` of the --stain_* flags, None for the default ``none``; ValueError for a bad value or an unreadable
    target (no GPU is touched)."""
    from .stain import StainNorm, check_parameters, load_target

    check_parameters(args.stain_alpha, args.stain_beta)  # checked whether or not the stage is on
    target = load_target(args.stain_target) if args.stain_target else None
    if args.stain_norm != "macenko":
        return None
    return StainNorm(alpha=args.stain_alpha, beta=args.stain_beta, target=target)


def normalize_stain(args, stain, tissue, slide):
    """--stain_norm macenko: right after the slide is opened, before anything reads its pixels (under --tissue_filter otsu the mask
    is made first, from the original pixels, and restricts the fit).  Nothing is read back here."""
    if stain is not None:
        stain.normalize(slide, tissue)


def report_stain(args, stain, tissue, slide):
    """The per-slide line of --stain_norm macenko (and the file of --stain_save_fit); called when the slide's results are back."""
    if stain is None:
        return
    fit = stain.normalize(slide, tissue)  # the fit the slide was normalised with
    print(f"[INFO] {slide.name}: {fit.report()}", flush=True)
    if args.stain_save_fit:
        import json

        fit_dir = os.path.join(os.getcwd(), "models", "first_model", "stain")
        os.makedirs(fit_dir, exist_ok=True)
        with open(os.path.join(fit_dir, slide.name + ".json"), "w") as f:
            json.dump({**fit.to_dict(), "alpha": stain.alpha, "beta": stain.beta}, f, indent=1)


def cmd_patch(args):
    from .dist import rank_world
    from .extract import save_patch_pngs, scan_level

    tissue = tissue_filter(args)
    stain = stain_norm(args)
    rank, world = rank_world()  # N > 1: every rank extracts the slides it owns; the outputs are per-slide directories
    for _, slide in open_slides(args, rank, world):
        normalize_stain(args, stain, tissue, slide)
        for level in levels_of(args):
            level_dir = os.path.join(data_root(args), "patches", f"level_{level}")
            save_dir = os.path.join(level_dir, slide.name)
            if os.path.isdir(save_dir) and os.listdir(save_dir):  # src/main.py:634-640
                print(f"[INFO] Patches for {slide.name} already extracted, skipping.")
                continue
            os.makedirs(save_dir, exist_ok=True)
            scan = scan_level(slide, level, stride=args.stride, tissue=tissue)
            np.savez(os.path.join(save_dir, "manifest.npz"), xy=scan.xy.cpu().numpy(),
                     keep=scan.keep.cpu().numpy(), labels=scan.labels.cpu().numpy(),
                     sums=scan.sums.cpu().numpy().astype(np.uint32), patch_size=scan.patch_size, level=level)
            n = int(scan.keep.sum().item())
            if args.write_png:
                if args.png_encoder == "host":
                    save_patch_pngs(slide, level, level_dir, stride=args.stride, tissue=tissue)
                else:
                    save_patch_pngs(slide, level, level_dir, stride=args.stride, tissue=tissue, encoder=args.png_encoder)
            print(f"[INFO] Patch extraction complete for {slide.name} at level {level}. Total patches: {n}")
        report_tissue(args, tissue, slide)
        report_stain(args, stain, tissue, slide)


def load_net(args, num_classes: Optional[int] = None):
    from . import capi, synth
    from .weights import canonical_state_dict

    if args.weights:
        sd = canonical_state_dict(torch.load(args.weights, map_location="cpu", weights_only=True))
    else:
        print("[WARNING] no --weights given: using seeded random-init ResNet18 "
              "(the reference's own transplant loads nothing either, SURVEY.md F4)")
        sd = synth.seeded_resnet18_state_dict(0, num_classes=num_classes)
    if num_classes is None:
        sd = {k: v for k, v in sd.items() if not k.startswith("fc.")}
    return capi.PackedResNet18(sd, precision=args.precision)


def cmd_extract_features(args):
    from .features import extract_features_from_pngs, save_feature_files

    level = int(args.patch_level) if args.patch_level != "all" else 3  # src/main.py:1134
    if args.simclr_encoder:  # extract_features_with_simclr: UnifiedResNet(encoder checkpoint, classifier=False)
        args.weights = args.simclr_encoder
    net = load_net(args, num_classes=None)
    patch_dir = os.path.join(data_root(args), "patches", f"level_{level}")
    has_png = os.path.isdir(patch_dir) and any(
        f.endswith(".png") for _, _, fs in os.walk(patch_dir) for f in fs)
    from .dist import rank_world, score_sharded
    from .extract import score_slide

    rank, world = rank_world()
    tissue = tissue_filter(args)
    stain = stain_norm(args)
    if has_png:
        if tissue is not None and rank == 0:
            print("[INFO] --tissue_filter otsu does not apply to a PNG patch tree: its patches were chosen when they were extracted")
        if stain is not None and rank == 0:
            print("[INFO] --stain_norm macenko does not apply to a PNG patch tree: its pixels were written when they were extracted")
        if world > 1 and rank == 0:
            print("[INFO] PNG patch tree: scored by rank 0 (the fused slide path is the one that shards)")
        if rank != 0:
            return 0
        feats, labels, paths = extract_features_from_pngs(patch_dir, net, batch_size=args.batch_size)
    else:
        # fused path: slides sharded over the ranks, one ragged all-gather, rows back in slide order -- the files rank 0
        # writes are the single-process files (DataParallel's gather order, src/main.py:841-842, :870-893)
        slides = list_slides(args)
        if not slides:
            print(f"[ERROR] Patches must be extracted at level {level} before extracting features.")
            return 1

        def score(i):
            slide = try_open(slides[i][0], slides[i][1])
            if slide is None:  # zero rows for this unit; the exchange and the other slides go on
                dev = torch.device("cuda", torch.cuda.current_device())
                return torch.zeros((0, 512), dtype=torch.float32, device=dev), None, torch.zeros((0, 4), dtype=torch.int32, device=dev)
            normalize_stain(args, stain, tissue, slide)
            f, _, _, meta = score_slide(slide, net, levels=(level,), batch_windows=512, stride=args.stride,
                                        want_logits=False, tissue=tissue)
            report_tissue(args, tissue, slide)
            report_stain(args, stain, tissue, slide)
            return f, None, meta

        f_all, _, meta = score_sharded(len(slides), score, rank, world)
        if rank != 0:
            return 0
        m = meta.cpu().numpy()
        feats, labels = f_all.cpu(), m[:, 3].astype(np.int64)
        names = [slides[u][0] for u in m[:, 4]]
        paths = [f"{n}/{n}_x{x}_y{y}_{'tumor' if lab else 'normal'}.png" for n, (x, y, lab) in zip(names, m[:, 1:4])]
    save_feature_files(level, feats.numpy(), labels, paths)
    print(f"[INFO] Features saved to patch_features_{level}.npy ({feats.shape[0]} patches)")
    return 0


def cmd_train(args, strategy: Optional[str]):
    from .train import train_resnet_classifier

    level = int(args.patch_level) if args.patch_level != "all" else 3
    patch_dir = os.path.join(data_root(args), "patches", f"level_{level}")
    hed = dict(hed_sigma=args.aug_hed, hed_seed=0 if args.seed is None else args.seed)
    if args.aug_hed > 0.0 and int(os.environ.get("RANK", "0")) == 0:
        from .augment_hed import describe

        print(f"[INFO] {describe(args.aug_hed)}", flush=True)
    if args.from_slides:
        # every rank holds every slide: batches are shared out, not slides (an unreadable file is skipped on every rank alike)
        slides = [s for s in (try_open(name, make) for name, make in list_slides(args)) if s is not None]
        train_resnet_classifier(None, strategy=strategy, epochs=args.epochs, batch_size=args.batch_size, precision=args.precision,
                                simclr_epochs=args.simclr_epochs, max_steps=args.max_steps, train_precision=args.train_precision,
                                simclr_precision=args.simclr_precision, slides=slides, level=level, **hed)
        return 0
    if not (os.path.isdir(patch_dir) and os.listdir(patch_dir)):
        print("[ERROR] Patches must be extracted before training.")
        return 1
    try:
        train_resnet_classifier(patch_dir, strategy=strategy, epochs=args.epochs, batch_size=args.batch_size,
                                precision=args.precision, simclr_epochs=args.simclr_epochs, max_steps=args.max_steps,
                                train_precision=args.train_precision, simclr_precision=args.simclr_precision,
                                device_aug=args.device_aug, **hed)
    except ValueError as e:
        if args.aug_hed > 0.0 and str(e).startswith("hed_sigma"):  # e.g. --device_aug fell back to the host transforms
            print(f"[ERROR] --aug_hed: {e}")
            return 2
        raise
    return 0


def detect_geometry(args):
    """The checked geometry and parameters of --detect, or None after a message (no GPU is touched)."""
    from . import detect

    try:
        geom = detect.geometry(args.detect_cell, levels_of(args))
        detect.check_parameters(args.detect_sigma, args.detect_radius, args.detect_max, args.detect_fuse)
    except ValueError as e:
        print(f"[ERROR] --detect: {e}")
        return None
    return geom


def cmd_detect(args):
    from . import detect
    from .dist import rank_world, shard_units

    geom = detect_geometry(args)
    if geom is None:
        return 2
    tissue = tissue_filter(args)
    stain = stain_norm(args)
    slides = list_slides(args, split="test")
    if not slides:
        print(f"[ERROR] No slides to detect on: '{os.path.join(data_root(args), 'test', 'img')}' holds none and no --synthetic was given.")
        return 1
    net = load_net(args, num_classes=2)
    csv_dir = os.path.join(os.getcwd(), "models", "first_model", "model_predictions_csv")
    map_dir = os.path.join(os.getcwd(), "models", "first_model", "heatmaps")
    os.makedirs(csv_dir, exist_ok=True)
    if args.detect_save_maps:
        os.makedirs(map_dir, exist_ok=True)
    rank, world = rank_world()  # N > 1: every rank detects on the slides it owns and writes their files
    tta_args = {"tta": args.detect_tta} if args.detect_tta != "none" else {}  # none: the call of before, argument for argument
    for i in shard_units(len(slides), rank, world):
        name = slides[i][0]
        slide = try_open(name, slides[i][1])
        if slide is None:
            continue
        normalize_stain(args, stain, tissue, slide)
        res = detect.detect_slide(slide, net, levels=geom.levels, cell=geom.cell, fuse=args.detect_fuse, sigma=args.detect_sigma,
                                  radius=args.detect_radius, threshold=args.detect_threshold, max_detections=args.detect_max,
                                  tissue=tissue, **tta_args)
        n = detect.save_detection_csv(os.path.join(csv_dir, name + ".csv"), res)
        if args.detect_save_maps:
            np.save(os.path.join(map_dir, name + ".npy"), res.fused.cpu().numpy())
            if tta_args:
                np.save(os.path.join(map_dir, name + "_tta_range.npy"), detect.range_map(res, args.detect_fuse).cpu().numpy())
        print(f"[INFO] {name}: {res.probs.shape[0]} windows at levels {list(geom.levels)}, map {res.grid[0]} x {res.grid[1]} cells of "
              f"{geom.cell} px, {n} detections" + (f", {res.views} views" if tta_args else ""), flush=True)
        report_tissue(args, tissue, slide)
        report_stain(args, stain, tissue, slide)
    return 0


def cmd_run_evaluation(args):
    from .dist import rank_world
    from .froc import run_evaluation

    rank, _ = rank_world()
    if rank != 0:  # the evaluation is not sharded: rank 0 does it
        return 0
    return run_evaluation(data_root(args), eval_roc=args.eval_roc, slide_scores=args.eval_slide_scores, bootstrap=args.eval_bootstrap,
                          ci=args.eval_ci, seed=0 if args.seed is None else args.seed)


def mil_triple(args):
    """(features, labels, paths) file names of the one level --patch_level names, or None after a message."""
    if args.patch_level == "all":
        print("[ERROR] --train_mil / --predict_mil work on one level: give --patch_level 0, 1, 2 or 3, not 'all'.")
        return None
    level = int(args.patch_level)
    triple = (f"patch_features_{level}.npy", f"patch_labels_{level}.npy", f"patch_paths_{level}.txt")
    missing = [f for f in triple if not os.path.exists(f)]
    if missing:
        print(f"[ERROR] {', '.join(missing)} not found: run --extract_features --patch_level {level} first.")
        return None
    return triple


def check_mil_args(parser, args):
    """The combinations of the MIL flags that are refused, as argparse errors (exit status 2), before anything else runs."""
    heads = args.mil_heads
    if heads is not None and not 1 <= heads <= 8:
        parser.error(f"--mil_heads {heads}: give 1 .. 8 attention heads")
    if heads is not None and heads > 1:
        if args.mil_pooling != "attention":
            parser.error(f"--mil_heads {heads} needs --mil_pooling attention: {args.mil_pooling} pooling has no attention to branch")
        if args.mil_dropout > 0.0 or args.mil_mc_samples > 0:
            parser.error(f"--mil_heads {heads} with --mil_dropout / --mil_mc_samples is not implemented: the dropout step and the "
                         "Monte-Carlo pass are single-head")
    if args.mil_gated:
        if args.mil_pooling != "attention":
            parser.error(f"--mil_gated needs --mil_pooling attention: {args.mil_pooling} pooling has no attention to gate")
        if args.mil_dropout > 0.0 or args.mil_mc_samples > 0:
            parser.error("--mil_gated with --mil_dropout / --mil_mc_samples is not implemented: the dropout step and the "
                         "Monte-Carlo pass are single-head and ungated")
    if args.mil_levels is not None:
        from .mil_levels import parse_levels_flag

        try:
            args.mil_levels = parse_levels_flag(args.mil_levels)
        except ValueError as e:
            parser.error(str(e))
        if args.mil_pooling != "attention":
            parser.error(f"--mil_levels needs --mil_pooling attention: {args.mil_pooling} pooling has no attention branch per level")
        if heads is not None and heads > 1:
            parser.error(f"--mil_levels with --mil_heads {heads} is not implemented: every level has one attention branch")
        if args.mil_gated:
            parser.error("--mil_levels with --mil_gated is not implemented: the branches of the levels are ungated")
        if args.mil_dropout > 0.0 or args.mil_mc_samples > 0:
            parser.error("--mil_levels with --mil_dropout / --mil_mc_samples is not implemented: the dropout step and the "
                         "Monte-Carlo pass are single-scale")
    if args.mil_save_attention and args.mil_pooling != "attention":
        parser.error(f"--mil_save_attention needs --mil_pooling attention: {args.mil_pooling} pooling has no attention weights")


def mil_model_levels(args):
    """The pyramid levels of the saved model of --predict_mil when it is a levels model (read on the host), else None."""
    if args.mil_pooling != "attention" or not os.path.exists(args.mil_model):
        return None
    from .mil_levels import LEVELS_KEY, model_levels

    try:
        sd = torch.load(args.mil_model, map_location="cpu", weights_only=True)
    except Exception:  # not a readable state_dict: the single-level path says so as it always did
        return None
    return model_levels(sd) if isinstance(sd, dict) and LEVELS_KEY in sd else None  # ValueError: the buffer against attn_U


def cmd_mil_levels(args, train: bool, levels):
    """--train_mil --mil_levels, and --predict_mil with a model trained that way: the triples of all its levels."""
    from .mil_levels import triple_names

    missing = [(level, f) for level in levels for f in triple_names(level) if not os.path.exists(f)]
    if missing:
        print(f"[ERROR] {', '.join(f for _, f in missing)} not found: run --extract_features --patch_level L for L in "
              f"{','.join(str(v) for v in sorted({v for v, _ in missing}))} first.")
        return 2
    from .dist import rank_world

    if rank_world()[0] != 0:  # not sharded: rank 0 does it
        return 0
    from . import mil_train

    seed = 0 if args.seed is None else args.seed
    try:
        if train:
            mil_train.train_mil(None, None, None, pooling="attention", epochs=args.mil_epochs, bags_per_step=args.mil_bags_per_step,
                                bag_size=args.mil_bag_size, seed=seed, max_steps=args.max_steps, levels=levels)
        else:
            mil_train.predict_mil(args.mil_model, None, None, None, pooling="attention", seed=seed, heads=args.mil_heads,
                                  save_attention=args.mil_save_attention, levels=args.mil_levels, dropout=args.mil_dropout,
                                  mc_samples=args.mil_mc_samples)
    except ValueError as e:  # differing feature dims; the model's levels against the flags
        print(f"[ERROR] --{'train_mil' if train else 'predict_mil'}: {e}")
        return 2
    return 0


def cmd_mil(args, train: bool):
    try:
        levels = args.mil_levels if train else mil_model_levels(args)
    except ValueError as e:  # a levels model whose buffer disagrees with its attention branches
        print(f"[ERROR] --predict_mil: {args.mil_model}: {e}")
        return 2
    if levels is not None:
        return cmd_mil_levels(args, train, levels)
    triple = mil_triple(args)  # before anything touches a GPU
    if triple is None:
        return 2
    if not 0.0 <= args.mil_dropout < 1.0:
        print(f"[ERROR] --mil_dropout {args.mil_dropout}: the probability must satisfy 0 <= P < 1.")
        return 2
    if not train and args.mil_mc_samples != 0:
        if not 0 < args.mil_mc_samples <= 4096:
            print(f"[ERROR] --mil_mc_samples {args.mil_mc_samples}: give 1 .. 4096 samples.")
            return 2
        if args.mil_dropout == 0.0:
            print("[ERROR] --mil_mc_samples needs --mil_dropout P with 0 < P < 1: without dropout every sample is the same forward.")
            return 2
    from .dist import rank_world

    if rank_world()[0] != 0:  # not sharded: rank 0 does it
        return 0
    from . import mil_train

    if train:
        mil_train.train_mil(*triple, pooling=args.mil_pooling, by_slide=args.mil_by_slide, epochs=args.mil_epochs,
                            bags_per_step=args.mil_bags_per_step, bag_size=args.mil_bag_size,
                            seed=0 if args.seed is None else args.seed, max_steps=args.max_steps, dropout=args.mil_dropout,
                            heads=1 if args.mil_heads is None else args.mil_heads, gated=args.mil_gated)
        return 0
    if not os.path.exists(args.mil_model):
        print(f"[ERROR] {args.mil_model} not found: run --train_mil first or give --mil_model PATH.")
        return 2
    try:
        mil_train.predict_mil(args.mil_model, *triple, pooling=args.mil_pooling, by_slide=args.mil_by_slide, dropout=args.mil_dropout,
                              mc_samples=args.mil_mc_samples, threshold=args.mil_threshold, seed=0 if args.seed is None else args.seed,
                              heads=args.mil_heads, save_attention=args.mil_save_attention, levels=args.mil_levels)
    except ValueError as e:  # the model's head count or its gate against the flags
        print(f"[ERROR] --predict_mil: {e}")
        return 2
    return 0


def cmd_validate(args) -> int:
    """--validate: the reference's validate_resnet_classifier (src/main.py:1017-1070) on the feature files of every level
    of --patch_level; validate.py has the driver."""
    import json

    from . import validate
    from .dist import rank_world

    if rank_world()[0] != 0:  # not sharded: rank 0 does it
        return 0
    if not args.validate_C > 0 or not args.validate_tol > 0:
        print("[ERROR] --validate_C and --validate_tol must be positive.")
        return 2
    rc = 0
    for level in levels_of(args):
        features_path = os.path.join(os.getcwd(), f"patch_features_{level}.npy")
        labels_path = os.path.join(os.getcwd(), f"patch_labels_{level}.npy")
        if not os.path.exists(features_path) or not os.path.exists(labels_path):
            print("[ERROR] Features or labels not found. Please run feature extraction first.")
            rc = 1
            continue
        features, labels = np.load(features_path), np.load(labels_path)
        print(f"[INFO] Feature shape: {features.shape}")
        print(f"[INFO] Labels shape: {labels.shape}")
        try:
            labels = validate.check_labels(labels)
            if features.ndim != 2 or features.shape[0] != labels.shape[0] or features.shape[0] == 0:
                raise ValueError(f"features {features.shape} and labels {labels.shape} do not agree")
            if features.shape[1] % 4 or not 4 <= features.shape[1] <= 2048:
                raise ValueError(f"feature dimension {features.shape[1]}: a multiple of 4 in 4..2048 is supported")
        except ValueError as e:
            print(f"[ERROR] --validate, level {level}: {e}.")
            rc = 2
            continue
        print(f"[INFO] Label distribution (0=normal, 1=tumor): {np.bincount(labels)}")
        res = validate.run(features, labels, seed=42 if args.seed is None else args.seed, C_reg=args.validate_C,
                           tol=args.validate_tol, knn_k=args.validate_knn or 0,
                           knn_temperature=0.07 if args.validate_knn_T is None else args.validate_knn_T)
        doc = validate.report(res)
        os.makedirs("results", exist_ok=True)
        with open(os.path.join("results", f"validate_{level}.json"), "w") as f:
            json.dump(doc, f, indent=2)
        if args.validate_save_pca:
            np.save(os.path.join("results", f"pca_{level}.npy"), res["projection"])
        if args.validate_save_knn and "knn" in res:
            np.save(os.path.join("results", f"knn_{level}.npy"), res["knn"]["neighbours"])
    return rc


def eval_patches_sources(args):
    """(weights path, level, patch_dir) of --eval_patches."""
    level = int(args.patch_level) if args.patch_level != "all" else 3  # as for --train
    weights = args.weights or os.path.join(os.getcwd(), "src", "models", "resnet18_patch_classifier.pth")  # src/main.py:978
    return weights, level, os.path.join(data_root(args), "patches", f"level_{level}")


def check_eval_patches_inputs(args, trained: bool = False, patched: bool = False) -> int:
    """0, or 1 after the reference's message for a missing checkpoint / a missing patch tree; no GPU is touched.  ``trained`` /
    ``patched``: the same invocation makes the file / the tree first, so its absence now means nothing."""
    weights, _, patch_dir = eval_patches_sources(args)
    if not trained and not os.path.exists(weights):
        print(f"[ERROR] Model file '{weights}' does not exist. Please train the model first.")
        return 1
    if args.from_slides:
        missing = not list_slides(args)
    else:
        missing = not patched and not (os.path.isdir(patch_dir) and any(f.endswith(".png") for _, _, fs in os.walk(patch_dir) for f in fs))
    if missing:
        print("[ERROR] Patches must be extracted before evaluation.")
        return 1
    return 0


def cmd_eval_patches(args) -> int:
    """--eval_patches: the reference's evaluate_resnet_classifier (src/main.py:974-1015); evaluate.py has the driver."""
    import json

    from . import evaluate
    from .dist import rank_world

    rc = check_eval_patches_inputs(args)
    if rc:
        return rc
    weights, level, patch_dir = eval_patches_sources(args)
    rank, world = rank_world()
    if world == 1 and args.seed is None:
        _seed_everything(0)  # the dataset's shuffle decides which patches the balancing keeps: two runs score the same set
    if rank == 0:
        print("[INFO] Evaluating ResNet18 classifier...", flush=True)
    slides = None
    if args.from_slides:  # every rank holds every slide: batches are shared out, not slides
        slides = [s for s in (try_open(name, make) for name, make in list_slides(args)) if s is not None]
    try:
        doc = evaluate.evaluate_patches(patch_dir, slides=slides, level=level, weights=weights, precision=args.precision,
                                        batch_size=args.batch_size, threshold=args.eval_threshold, unbalanced=args.eval_unbalanced,
                                        bootstrap=args.eval_bootstrap, ci=args.eval_ci, seed=0 if args.seed is None else args.seed,
                                        device_aug=args.device_aug)
    except evaluate.EvaluateError as e:
        print(f"[ERROR] --eval_patches: {e}")
        return e.status
    if doc is None:  # not rank 0
        return 0
    (tn, fp), (fn, tp) = doc["confusion_matrix"]
    print(f"[INFO] Classifier accuracy on validation patches: {doc['accuracy']:.4f}")
    print(f"[INFO] Confusion matrix over {doc['n']} patches of {len(doc['per_slide'])} slides: TN {tn}, FP {fp}, FN {fn}, TP {tp}")
    for line in evaluate.bootstrap_lines(doc) if "bootstrap" in doc else ():
        print(line)
    os.makedirs("results", exist_ok=True)
    with open(os.path.join("results", f"evaluate_{level}.json"), "w") as f:
        json.dump(doc, f, indent=1)
    print(f"[INFO] Results written to results/evaluate_{level}.json")
    return 0


def _seed_everything(seed: int):
    import random

    random.seed(seed)
    np.random.seed(seed & 0x7FFFFFFF)
    torch.manual_seed(seed)


def main(argv=None) -> int:
    argv = list(sys.argv[1:] if argv is None else argv)
    parser = build_parser()
    args = parser.parse_args(argv)
    check_mil_args(parser, args)
    check_aug_args(parser, args)
    check_eval_patches_args(parser, args)
    check_png_args(parser, args)
    check_tta_args(parser, args)
    check_validate_knn_args(parser, args)
    for name in OUT_OF_SCOPE:
        if getattr(args, name):
            print(f"[ERROR] --{name} is outside the accelerated hot path (see DESIGN.md 'Out of scope').")
            return 2
    if (args.train_mil or args.predict_mil) and args.patch_level == "all" and args.mil_levels is None:
        mil_triple(args)  # prints why; refused before any process is started or any GPU touched
        return 2
    if args.detect and detect_geometry(args) is None:  # refused before any process is started or any GPU touched
        return 2
    try:
        tissue_filter(args)  # likewise
    except ValueError as e:
        print(f"[ERROR] --tissue_filter: {e}")
        return 2
    try:
        stain_norm(args)  # likewise
    except ValueError as e:
        print(f"[ERROR] --stain_norm: {e}")
        return 2
    if args.eval_patches and check_eval_patches_inputs(args, trained=args.train or args.train_strategy, patched=args.patch):
        return 1  # refused before any process is started or any GPU touched
    under_launcher = "WORLD_SIZE" in os.environ and "RANK" in os.environ
    if args.world_size > 1 and not under_launcher:
        # parent: start one fresh process per GPU and supervise them; nothing here may initialise the GPU
        from . import launch

        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))  # importable from any working directory
        entry = ["-c", f"import sys; sys.path.insert(0, {root!r}); from {__package__}.main import main; sys.exit(main())"]
        cmds = launch.child_commands(entry, argv, args.world_size, launch.free_port())
        return launch.launch_ranks(cmds, rank_timeout=args.rank_timeout, name="main.py")
    if under_launcher and int(os.environ["WORLD_SIZE"]) > 1:
        from . import dist as hdist

        rank, world, local = hdist.init_from_env(args.dist_backend)
        if args.world_size not in (1, world):
            print(f"[ERROR] --world_size {args.world_size} but WORLD_SIZE={world}")
            return 2
        torch.cuda.set_device(0 if args.one_device else local)
        _seed_everything(0 if args.seed is None else args.seed)  # the same host-side draws on every rank
    elif args.seed is not None:
        _seed_everything(args.seed)
    try:
        return _dispatch(args)
    finally:
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            torch.distributed.destroy_process_group()


def _rendezvous():
    """--world_size N: the commands of one invocation run back to back on every rank, and the next one lists what the
    previous one wrote (the PNG tree, the feature files): nobody moves on before everybody is done.  Also keeps the ranks
    that sit out a rank-0-only phase (the PNG branch of --extract_features) out of the next command's collectives."""
    if torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1:
        torch.distributed.barrier()


def _dispatch(args) -> int:
    rc = 0
    if args.patch:
        cmd_patch(args)
        _rendezvous()
    if args.extract_features:
        rc = cmd_extract_features(args) or rc
        _rendezvous()
    if args.train:
        rc = cmd_train(args, None) or rc
    if args.train_strategy:
        rc = cmd_train(args, args.strategy) or rc
    if args.eval_patches:
        _rendezvous()  # rank 0 of --train wrote the checkpoint
        rc = cmd_eval_patches(args) or rc
    if args.detect:
        rc = cmd_detect(args) or rc
        _rendezvous()  # --run_evaluation on rank 0 reads every rank's CSVs
    if args.run_evaluation:
        rc = cmd_run_evaluation(args) or rc
    if args.train_mil:
        _rendezvous()
        rc = cmd_mil(args, True) or rc
    if args.predict_mil:
        rc = cmd_mil(args, False) or rc
    if args.validate:
        rc = cmd_validate(args) or rc
    return rc


if __name__ == "__main__":
    sys.exit(main())
