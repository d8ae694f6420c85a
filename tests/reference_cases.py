"""Seeded cases shared by tests/test_reference_parity.py and
tools/make_reference_golden.py.

Every case builds this framework's module from a fixed seed, draws its
inputs from a second fixed seed and returns a dict of named results. Called
with `ref=None` it runs this framework. Called with a `Reference` (the
generator only) it builds the reference implementation's class, loads the
SAME weights into it and returns the reference's results; those are what is
stored under tests/golden/reference_parity/. No reference code lives here:
the reference is imported as an external oracle from a directory the
generator is given.
"""

import argparse
import importlib
import sys

import numpy as np
import torch

GRAD_SAMPLE = 384  # elements kept of every parameter gradient
GRAD_SEED = 77


class Reference:
    """Imports the reference's modules from its `core` directory."""

    def __init__(self, core_dir):
        self.core_dir = core_dir

    def mod(self, name):
        sys.path.insert(0, self.core_dir)
        try:
            return importlib.import_module(name)
        finally:
            sys.path.remove(self.core_dir)


def _shared(ref, our_cls, ref_mod, *a, **kw):
    """Our module, or the reference's same-named class with our weights."""
    o = our_cls(*a, **kw)
    if ref is None:
        return o
    rng = torch.get_rng_state()  # later draws must not depend on `ref`
    r = getattr(ref.mod(ref_mod), our_cls.__name__)(*a, **kw)
    torch.set_rng_state(rng)
    r.load_state_dict(o.state_dict())
    return r


def _model(ref, args, ref_mod):
    from flowhip.models import build_model
    o = build_model(args)
    if ref is None:
        return o
    rng = torch.get_rng_state()
    r = ref.mod(ref_mod).RAFT(args)
    torch.set_rng_state(rng)
    r.load_state_dict(o.state_dict())
    return r


def ncup_args(**kw):
    from flowhip.config.args import default_ncup_args
    args = default_ncup_args(model="raft_nc_dbl", **kw)
    args.mixed_precision = False
    return args


def raft_args(small):
    from flowhip.config.args import default_ncup_args
    args = default_ncup_args(model="raft", small=small)
    args.mixed_precision = False
    args.align_corners = False  # reference train.py:294 flag (accessed by ref)
    return args


def _images():
    torch.manual_seed(100)
    return (torch.rand(1, 3, 128, 128) * 255, torch.rand(1, 3, 128, 128) * 255)


def grad_sample_index(numel):
    g = torch.Generator().manual_seed(GRAD_SEED + numel)
    return torch.randperm(numel, generator=g)[:GRAD_SAMPLE]


# ---------------------------------------------------------------- surfaces

def state_dict_surface(ref, which):
    """key -> shape of the full models (`ncup`, `raft_small`, `raft_basic`)."""
    if which == "ncup":
        m = _model(ref, ncup_args(), "raft_nc_dbl")
    else:
        m = _model(ref, raft_args(which == "raft_small"), "raft")
    return {k: list(v.shape) for k, v in m.state_dict().items()}


def reflective_flags(ref):
    """Option names of the three reflective module families."""
    if ref is None:
        from flowhip.config import build_train_parser
        ours = build_train_parser(argv=[])
        return sorted(o for a in ours._actions for o in a.option_strings
                      if o.startswith(("--final_upsampling", "--interp_net",
                                       "--weights_est_net")))
    # the reference's introspection machinery, driven as its train.py does
    saved_argv = sys.argv
    sys.argv = ["x", "--final_upsampling", "NConvUpsampler",
                "--interp_net", "NConvUNet", "--weights_est_net", "Simple"]
    try:
        ra = ref.mod("utils.args")
        parser = argparse.ArgumentParser()
        ra._add_arguments_for_module(
            parser, ref.mod("upsampler"), name="final_upsampling",
            default_class=None, exclude_classes=["_*"],
            exclude_params=["self", "args", "interpolation_net",
                            "weights_est_net", "size"],
            forced_default_types={"scale": int,
                                  "use_data_for_guidance": ra.str2bool,
                                  "channels_to_batch": ra.str2bool,
                                  "use_residuals": ra.str2bool,
                                  "est_on_high_res": ra.str2bool})
        ra._add_arguments_for_module(
            parser, ref.mod("nconv_modules"), name="interp_net",
            default_class=None, exclude_classes=["_*"],
            exclude_params=["self", "args"],
            forced_default_types={"encoder_fiter_sz": int,
                                  "decoder_fiter_sz": int,
                                  "out_filter_size": int,
                                  "use_double_conv": ra.str2bool,
                                  "use_bias": ra.str2bool})
        ra._add_arguments_for_module(
            parser, ref.mod("interp_weights_est"), name="weights_est_net",
            default_class=None, exclude_classes=["_*"],
            exclude_params=["self", "args", "out_ch", "final_act"],
            unknown_default_types={"num_ch": ra.str2intlist,
                                   "filter_sz": ra.str2intlist},
            forced_default_types={"dilation": ra.str2intlist})
    finally:
        sys.argv = saved_argv
    return sorted(o for a in parser._actions for o in a.option_strings
                  if o.startswith("--") and o != "--help")


def raft_small_outcome(ref):
    """What RAFT-small's forward does: result shape, or the exception name."""
    torch.manual_seed(0)
    m = _model(ref, raft_args(True), "raft")
    img1, img2 = _images()
    try:
        out = m(img1, img2, iters=2)
    except Exception as e:  # noqa: BLE001 - the outcome is the datum
        return {"raises": type(e).__name__}
    return {"raises": None, "n": len(out), "shape": list(out[-1].shape)}


# ------------------------------------------------------------ full models

def ncup_forward_and_grads(ref):
    """3 refinement iterations at the minimum supported size, train mode:
    the predictions, and of every parameter gradient its norm and a seeded
    sample of GRAD_SAMPLE elements."""
    torch.manual_seed(0)
    m = _model(ref, ncup_args(), "raft_nc_dbl")
    m.train()
    img1, img2 = _images()
    preds = m(img1, img2, iters=3)
    out = {"pred%d" % i: p.detach() for i, p in enumerate(preds)}
    sum(p.abs().mean() for p in preds).backward()
    for name, p in m.named_parameters():
        if p.grad is None:
            continue
        g = p.grad.reshape(-1)
        out["gnorm:" + name] = g.norm().reshape(1)
        out["gsample:" + name] = g[grad_sample_index(g.numel())].clone()
    return out


def raft_basic_forward(ref):
    torch.manual_seed(0)
    m = _model(ref, raft_args(False), "raft")
    img1, img2 = _images()
    preds = m(img1, img2, iters=2)
    out = {"pred%d" % i: p.detach() for i, p in enumerate(preds)}
    low, up = m(img1, img2, iters=2, test_mode=True)
    out["low"], out["up"] = low.detach(), up.detach()
    return out


# ------------------------------------------------------------- components

def nconv_unet(ref, shared, pool):
    from flowhip.nn.nconv import NConvUNet
    torch.manual_seed(1)
    m = _shared(ref, NConvUNet, "nconv_modules", in_ch=1,
                channels_multiplier=2, num_downsampling=3,
                shared_encoder=shared, data_pooling=pool)
    torch.manual_seed(101)
    data = torch.randn(2, 1, 64, 64)
    conf = torch.rand(2, 1, 64, 64) * (torch.rand(2, 1, 64, 64) > 0.5)
    x, c = m((data, conf))
    return {"x": x.detach(), "c": c.detach()}


def pac_ops(ref):
    from flowhip.nn import pac as our_pac
    from flowhip.nn import pac_upsampler as our_pup
    pac = ref.mod("pac_modules") if ref else our_pac
    torch.manual_seed(0)
    guide = torch.randn(2, 4, 16, 16)
    x = torch.randn(2, 6, 16, 16)
    w = torch.randn(8, 6, 3, 3)
    b = torch.randn(8)
    k, _ = pac.packernel2d(guide, kernel_size=3, stride=1, padding=1,
                           dilation=1)
    y = pac.pacconv2d(x, k, w, b, stride=1, padding=1, dilation=1)
    out = {"kernel": k, "conv": y}

    torch.manual_seed(102)
    lr = torch.randn(2, 1, 8, 8)
    hr_guide = torch.randn(2, 3, 32, 32)
    torch.manual_seed(2)
    up = _shared(ref, our_pup.PacJointUpsample, "pac_upsampler", factor=4,
                 channels=1, guide_channels=3)
    out["joint"] = up(lr, hr_guide).detach()
    torch.manual_seed(3)
    dj = _shared(ref, our_pup.DJIF, "pac_upsampler", factor=4, channels=1,
                 guide_channels=3)
    out["djif"] = dj(lr, hr_guide).detach()
    return out


def pac_gradients(ref):
    from flowhip.nn import pac as our_pac
    pac = ref.mod("pac_modules") if ref else our_pac
    torch.manual_seed(0)
    guide = torch.randn(2, 4, 10, 10)
    x = torch.randn(2, 6, 10, 10)
    w = torch.randn(5, 6, 3, 3)
    b = torch.randn(5)
    ins = [t.clone().requires_grad_(True) for t in (guide, x, w, b)]
    k, _ = pac.packernel2d(ins[0], kernel_size=3, stride=1, padding=1,
                           dilation=1)
    y = pac.pacconv2d(ins[1], k, ins[2], ins[3], stride=1, padding=1,
                      dilation=1)
    grads = torch.autograd.grad(y.square().sum(), ins)
    return dict(zip(["dguide", "dx", "dw", "db"], grads))


def pac_transpose_pool(ref):
    from flowhip.nn import pac as our_pac
    torch.manual_seed(0)
    t = _shared(ref, our_pac.PacConvTranspose2d, "pac_modules", 4, 5,
                kernel_size=5, stride=2, padding=2, output_padding=1)
    p = _shared(ref, our_pac.PacPool2d, "pac_modules", kernel_size=3,
                stride=2, padding=1)
    torch.manual_seed(103)
    x = torch.randn(2, 4, 8, 8)
    guide = torch.randn(2, 3, 16, 16)
    xp = torch.randn(2, 4, 16, 16)
    gp = torch.randn(2, 4, 16, 16)
    return {"transpose": t(x, guide).detach(), "pool": p(xp, gp).detach()}


def flow_viz(ref):
    from flowhip.data import flow_viz as our_viz
    viz = ref.mod("utils.flow_viz") if ref else our_viz
    rng = np.random.default_rng(0)
    flow = (rng.standard_normal((16, 20, 2)) * 10).astype(np.float32)
    return {"color": viz.flow_to_color(flow.copy()),
            "image": viz.flow_to_image(flow.copy())}


def geometry(ref):
    from flowhip.utils import geometry as ours
    g = ref.mod("utils.utils") if ref else ours
    torch.manual_seed(0)
    out = {}
    for mode in ("sintel", "kitti"):
        # 61 and 53 leave the same remainders mod 8 as Sintel's 437 x 1021
        x = torch.randn(2, 3, 61, 53)
        padder = g.InputPadder(x.shape, mode=mode)
        a = padder.pad(x.clone())[0]
        out[mode + "_pad"] = a
        out[mode + "_unpad"] = padder.unpad(a)
    img = torch.randn(4, 2, 17, 23)
    coords = torch.rand(4, 9, 11, 2) * 25 - 1  # includes out-of-bounds
    out["bilinear"] = g.bilinear_sampler(img, coords)
    out["grid"] = g.coords_grid(2, 7, 9)
    out["upflow8"] = g.upflow8(torch.randn(1, 2, 6, 8))
    fl = torch.randn(2, 12, 14) * 3
    out["forward_interpolate"] = g.forward_interpolate(fl.clone())
    return out


def extractors(ref, norm):
    from flowhip.nn import extractor as our_ext
    out = {}
    for cls, dim in ((our_ext.BasicEncoder, 64), (our_ext.SmallEncoder, 32)):
        torch.manual_seed(1)
        m = _shared(ref, cls, "extractor", output_dim=dim, norm_fn=norm,
                    dropout=0.0)
        m.eval()
        torch.manual_seed(104)
        with torch.no_grad():
            out[cls.__name__] = m(torch.randn(2, 3, 64, 64))
    return out


def update_blocks(ref):
    from flowhip.config.args import default_ncup_args
    from flowhip.nn import update as our_upd
    out = {}
    for small, cls, radius, hidden, ctx in (
            (True, our_upd.SmallUpdateBlock, 3, 96, 64),
            (False, our_upd.BasicUpdateBlock, 4, 128, 128)):
        torch.manual_seed(0)
        args = default_ncup_args(model="raft", small=small)
        # set by RAFT.__init__ (raft.py:28-29, 33-34)
        args.corr_levels, args.corr_radius = 4, radius
        cor_planes = args.corr_levels * (2 * radius + 1) ** 2
        m = _shared(ref, cls, "update", args, hidden_dim=hidden)
        torch.manual_seed(105)
        net = torch.randn(2, hidden, 8, 8)
        inp = torch.randn(2, ctx, 8, 8)
        corr = torch.randn(2, cor_planes, 8, 8)
        flow = torch.randn(2, 2, 8, 8)
        with torch.no_grad():
            net_o, mask, dflow = m(net, inp, corr, flow)
        n = cls.__name__
        out[n + "_net"], out[n + "_dflow"] = net_o, dflow
        out[n + "_has_mask"] = np.array([int(mask is not None)])
        if mask is not None:
            out[n + "_mask"] = mask
    return out


def unet_weights_est(ref):
    from flowhip.nn import interp_weights_est as our_iwe
    torch.manual_seed(1)
    m = _shared(ref, our_iwe.UNet, "interp_weights_est",
                num_ch=[5, 8, 12, 16], out_ch=1)
    m.eval()
    torch.manual_seed(106)
    with torch.no_grad():
        return {"y": m(torch.randn(2, 5, 32, 32))}


NCUP_HEAD_CASES = [
    (5, dict(use_data_for_guidance=True, channels_to_batch=True,
             use_residuals=False)),
    (5, dict(use_data_for_guidance=True, channels_to_batch=True,
             use_residuals=True)),
    (4, dict(use_data_for_guidance=False, channels_to_batch=False,
             use_residuals=False)),
    (0, dict(use_data_for_guidance=False)),  # binary-weights fallback
]


def nconv_upsampler_head(ref, index):
    from flowhip.nn import upsampler as our_up
    from flowhip.nn.interp_weights_est import Simple
    from flowhip.nn.nconv import NConvUNet
    weights_in, kw = NCUP_HEAD_CASES[index]
    torch.manual_seed(3)
    inet = _shared(ref, NConvUNet, "nconv_modules", in_ch=1,
                   channels_multiplier=2, num_downsampling=1)
    w = None
    if weights_in:
        w = _shared(ref, Simple, "interp_weights_est",
                    num_ch=[weights_in, 8], out_ch=1, filter_sz=[3, 1],
                    dilation=[1, 1], final_act=torch.sigmoid)
    cls = (ref.mod("upsampler") if ref else our_up).NConvUpsampler
    m = cls(scale=4, interpolation_net=inet, weights_est_net=w, **kw)
    torch.manual_seed(4)
    lr = torch.rand(2, 1, 8, 8) * (torch.rand(2, 1, 8, 8) > 0.6)
    guide = (lr.new_ones(2, 1, 32, 32) if weights_in == 0
             else torch.randn(2, 4, 32, 32))
    return {"y": m(lr.clone(), guide.clone()).detach()}


def pac_upsampler_heads(ref):
    from flowhip.nn import pac_upsampler as our_pup
    pup = ref.mod("pac_upsampler") if ref else our_pup
    torch.manual_seed(0)
    lr = torch.randn(2, 1, 8, 8)
    guide = torch.randn(2, 3, 32, 32)
    a = torch.randn(2, 2, 16, 16)
    b = torch.randn(2, 2, 16, 16)
    out = {}
    for name in ("PacJointUpsampleLite", "DJIFWide"):
        torch.manual_seed(5)
        m = _shared(ref, getattr(our_pup, name), "pac_upsampler", factor=4,
                    channels=1, guide_channels=3)
        out[name] = m(lr, guide).detach()
    m = _shared(ref, our_pup.JointBilateral, "pac_upsampler", factor=4,
                channels=1, kernel_size=5, scale_space=0.2, scale_color=5.0)
    out["JointBilateral"] = m(lr, guide).detach()
    out["Bilinear"] = pup.Bilinear(factor=4)(lr, guide)
    out["th_epe"] = pup.th_epe(a, b).reshape(-1)
    return out


def enforce_pos_hook(ref):
    """weight_p initialisation (the pos(weight) quirk), the effective weight
    and output after a parameter update."""
    from flowhip.nn import nconv as our_nc
    nc = ref.mod("nconv_modules") if ref else our_nc
    torch.manual_seed(31)
    w0 = torch.randn(3, 2, 3, 3)
    x = torch.randn(1, 2, 8, 8)
    m = torch.nn.Conv2d(2, 3, 3, bias=False)
    with torch.no_grad():
        m.weight.copy_(w0)
    nc.EnforcePos.apply(m, "weight", "softplus")
    out = {"weight_p_init": m.weight_p.detach().clone()}
    with torch.no_grad():
        m.weight_p.add_(0.25)
    out["y"] = m(x).detach()
    out["weight"] = m.weight.detach().clone()
    return out


# name -> (function, extra arguments); one .npz each under the golden folder
ARRAY_CASES = {
    "ncup_forward_and_grads": (ncup_forward_and_grads, ()),
    "raft_basic_forward": (raft_basic_forward, ()),
    "pac_ops": (pac_ops, ()),
    "pac_gradients": (pac_gradients, ()),
    "pac_transpose_pool": (pac_transpose_pool, ()),
    "flow_viz": (flow_viz, ()),
    "geometry": (geometry, ()),
    "update_blocks": (update_blocks, ()),
    "unet_weights_est": (unet_weights_est, ()),
    "pac_upsampler_heads": (pac_upsampler_heads, ()),
    "enforce_pos_hook": (enforce_pos_hook, ()),
}
for _s in (True, False):
    for _p in ("conf_based", "max_pooling"):
        ARRAY_CASES["nconv_unet_%s_%s" % (_s, _p)] = (nconv_unet, (_s, _p))
for _n in ("batch", "group", "instance", "none"):
    ARRAY_CASES["extractors_" + _n] = (extractors, (_n,))
for _i in range(len(NCUP_HEAD_CASES)):
    ARRAY_CASES["nconv_upsampler_head_%d" % _i] = (nconv_upsampler_head, (_i,))

# name -> (function, extra arguments); all in one surfaces.json
JSON_CASES = {
    "state_dict_ncup": (state_dict_surface, ("ncup",)),
    "state_dict_raft_small": (state_dict_surface, ("raft_small",)),
    "state_dict_raft_basic": (state_dict_surface, ("raft_basic",)),
    "reflective_flags": (reflective_flags, ()),
    "raft_small_outcome": (raft_small_outcome, ()),
}


def run_arrays(name, ref=None):
    fn, extra = ARRAY_CASES[name]
    out = fn(ref, *extra)
    return {k: (v.detach().cpu().numpy() if torch.is_tensor(v)
                else np.asarray(v)) for k, v in out.items()}


def run_json(name, ref=None):
    fn, extra = JSON_CASES[name]
    return fn(ref, *extra)
