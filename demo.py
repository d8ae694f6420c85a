#!/usr/bin/env python3
"""Inference demo on a directory of frames (reference demo.py:50-79).

Runs the model over consecutive frame pairs and writes flow visualizations
as PNGs (this image has no display; the reference used cv2.imshow).
As in the reference, --model is the CHECKPOINT path; the architecture is
selected with --arch (reference hardcoded RAFT).

    python demo.py --model ckpt.pth --path frames_dir [--out demo_out]
                   [--warm_start] [--bidirectional]

--bidirectional estimates both directions of every pair in one pass and
writes, per pair, flow_%04d.png (1->2), flow_bw_%04d.png (2->1) and
occ_%04d.png: the forward-backward occlusion mask of the 1->2 flow as an
8-bit image, 255 = occluded (`ops.fb_consistency` on the unpadded flows). One
log line per pair gives the visible share and the mean visible residual.
"""

import argparse
import glob
import os

import numpy as np
import torch
from PIL import Image

from flowhip import ops
from flowhip.config import add_ncup_module_flags, finalize_args
from flowhip.data import flow_viz
from flowhip.engine import checkpoints
from flowhip.engine.stream import FlowStream
from flowhip.models import build_model
from flowhip.utils.geometry import InputPadder
from flowhip.utils.geometry import InputPadder

DEVICE = "cuda" if torch.cuda.is_available() else "cpu"


def load_image(imfile):
    img = np.array(Image.open(imfile)).astype(np.uint8)
    img = torch.from_numpy(img).permute(2, 0, 1).float()
    return img[None].to(DEVICE)


def load_image_list(image_files):
    """Batch-load + pad a sorted frame list (reference demo.py:26-35)."""
    images = torch.cat([load_image(f) for f in sorted(image_files)], dim=0)
    padder = InputPadder(images.shape)
    return padder.pad(images)[0]


def viz(img, flo, out_path):
    img = img[0].permute(1, 2, 0).cpu().numpy()
    flo = flo[0].permute(1, 2, 0).cpu().numpy()
    flo = flow_viz.flow_to_image(flo)
    img_flo = np.concatenate([img, flo], axis=0).astype(np.uint8)
    Image.fromarray(img_flo).save(out_path)


def write_occlusion(flow_fw, flow_bw, out_path):
    """Forward-backward check of one unpadded pair: writes the 1->2 occlusion
    mask (255 = occluded) and returns the log line."""
    occ_fw, _, _, _, stats = ops.fb_consistency(flow_fw, flow_bw)
    Image.fromarray((occ_fw[0, 0] * 255).cpu().numpy()).save(out_path)
    npix = flow_fw.shape[-2] * flow_fw.shape[-1]
    visible, _, _, rsum = stats[0].cpu().unbind(-1)     # (fw, bw) each
    mean = rsum / visible.clamp(min=1)
    return ("%s: visible %.1f%% fw / %.1f%% bw, mean visible residual "
            "%.3f px fw / %.3f px bw"
            % (os.path.basename(out_path), 100 * visible[0] / npix,
               100 * visible[1] / npix, mean[0], mean[1]))


def demo(args):
    model_args = finalize_args(args)
    model_args.model = args.arch
    model = build_model(model_args)
    if args.model and os.path.exists(args.model):
        checkpoints.load_weights(model, args.model)
    model.to(DEVICE)
    model.eval()

    os.makedirs(args.out, exist_ok=True)
    with torch.no_grad():
        files = sorted(glob.glob(os.path.join(args.path, "*.png"))
                       + glob.glob(os.path.join(args.path, "*.jpg")))
        images = [load_image(f) for f in files]

        # --warm_start: the frames are one sequence; each pair starts from
        # the previous pair's flow, splatted forward on the device
        stream = FlowStream(model, iters=20, warm_start=args.warm_start,
                            bidirectional=args.bidirectional)
        for i, (image1, image2) in enumerate(zip(images[:-1], images[1:])):
            padder = InputPadder(image1.shape)
            image1, image2 = padder.pad(image1, image2)
            flow_low, flow_up = stream.step(image1, image2)
            if not args.bidirectional:
                viz(image1, flow_up,
                    os.path.join(args.out, "flow_%04d.png" % i))
                continue
            n = image1.shape[0]
            viz(image1, flow_up[:n],
                os.path.join(args.out, "flow_%04d.png" % i))
            viz(image2, flow_up[n:],
                os.path.join(args.out, "flow_bw_%04d.png" % i))
            print(write_occlusion(
                padder.unpad(flow_up[:n]), padder.unpad(flow_up[n:]),
                os.path.join(args.out, "occ_%04d.png" % i)))


def build_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument("--model", help="checkpoint path")
    parser.add_argument("--arch", default="raft", help="model architecture")
    parser.add_argument("--path", help="directory of frames")
    parser.add_argument("--out", default="demo_out")
    parser.add_argument("--small", action="store_true")
    parser.add_argument("--mixed_precision", action="store_true")
    parser.add_argument("--alternate_corr", action="store_true",
                        help="on-demand correlation lookup (no all-pairs "
                        "volume; for frames larger than memory allows)")
    parser.add_argument("--warm_start", action="store_true",
                        help="treat the frames as one sequence: start each "
                        "pair from the previous pair's flow (device-side "
                        "nearest splat)")
    parser.add_argument("--bidirectional", action="store_true",
                        help="estimate both directions of every pair and "
                        "write the backward flow and the forward-backward "
                        "occlusion mask (255 = occluded) next to the flow")
    add_ncup_module_flags(parser)
    return parser


if __name__ == "__main__":
    demo(build_parser().parse_args())
