"""GPU kernel tests (MI355X): HIP kernels vs the pure-torch fp32 oracle
(SURVEY.md §4.2 item 2). Run via gpurun: pytest tests -m gpu."""

import math

import pytest
import torch

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ext():
    import flowhip._C as C
    return C


class TestBgemmNT:
    def test_square_multiple_of_tile(self, ext):
        torch.manual_seed(0)
        a = torch.randn(2, 256, 256, device=_dev()).to(torch.bfloat16)
        b = torch.randn(2, 256, 256, device=_dev()).to(torch.bfloat16)
        c = ext.bgemm_nt(a, b, 0.5)
        ref = 0.5 * torch.matmul(a.float(), b.float().transpose(1, 2))
        assert c.shape == ref.shape
        torch.testing.assert_close(c, ref, atol=2e-3, rtol=2e-3)

    def test_ragged_edges(self, ext):
        # M, N not multiples of 128 (FlyingChairs P=2852 case)
        torch.manual_seed(1)
        a = torch.randn(1, 300, 128, device=_dev()).to(torch.bfloat16)
        b = torch.randn(1, 177, 128, device=_dev()).to(torch.bfloat16)
        c = ext.bgemm_nt(a, b, 1.0)
        ref = torch.matmul(a.float(), b.float().transpose(1, 2))
        torch.testing.assert_close(c, ref, atol=2e-3, rtol=2e-3)

    def test_asymmetric_catches_transpose(self, ext):
        # asymmetric operands catch a row/col swap (guide §3 A=I-check)
        a = torch.zeros(1, 128, 64, device=_dev())
        a[0, 3, :] = 1.0
        b = torch.zeros(1, 128, 64, device=_dev())
        b[0, 7, 0] = 2.0
        c = ext.bgemm_nt(a.to(torch.bfloat16), b.to(torch.bfloat16), 1.0)
        assert c[0, 3, 7].item() == pytest.approx(2.0, abs=1e-2)
        assert c[0, 7, 3].item() == 0.0


@pytest.fixture
def fp32_corr():
    """Pin the corr stack to the fp32-resident mode for exact-contract
    oracle tests (the default is the bf16-resident pyramid)."""
    from flowhip.utils import layout
    old = layout.corr_bf16_enabled()
    layout.set_corr_bf16(False)
    yield
    layout.set_corr_bf16(old)


class TestCorrVolume:
    def test_forward_matches_ref(self, fp32_corr):
        from flowhip.ops import torch_ref
        from flowhip.ops.functional import CorrVolumeFn
        torch.manual_seed(2)
        B, D, H, W = 2, 256, 14, 32
        f1 = torch.randn(B, D, H, W, device=_dev())
        f2 = torch.randn(B, D, H, W, device=_dev())
        out = CorrVolumeFn.apply(f1, f2)
        ref = torch_ref.corr_volume(f1, f2)
        assert out.shape == ref.shape
        # bf16 inputs, fp32 accumulate: |err| ~ sqrt(D)*eps_bf16*|f|^2
        torch.testing.assert_close(out, ref, atol=5e-2, rtol=5e-2)

    def test_backward_matches_ref(self, fp32_corr):
        from flowhip.ops import torch_ref
        from flowhip.ops.functional import CorrVolumeFn
        torch.manual_seed(3)
        B, D, H, W = 1, 128, 10, 23  # P=230: exercises K padding in backward
        f1 = torch.randn(B, D, H, W, device=_dev(), requires_grad=True)
        f2 = torch.randn(B, D, H, W, device=_dev(), requires_grad=True)

        out = CorrVolumeFn.apply(f1, f2)
        g = torch.randn_like(out)
        d1, d2 = torch.autograd.grad(out, (f1, f2), g)

        f1r = f1.detach().clone().requires_grad_(True)
        f2r = f2.detach().clone().requires_grad_(True)
        ref = torch_ref.corr_volume(f1r, f2r)
        r1, r2 = torch.autograd.grad(ref, (f1r, f2r), g)

        torch.testing.assert_close(d1, r1, atol=0.5, rtol=5e-2)
        torch.testing.assert_close(d2, r2, atol=0.5, rtol=5e-2)


class TestCorrLookup:
    @pytest.mark.parametrize("radius", [3, 4])
    def test_forward_matches_ref(self, radius):
        from flowhip import ops
        from flowhip.ops import torch_ref
        from flowhip.ops.functional import CorrLookupFn
        torch.manual_seed(4)
        B, H, W = 1, 16, 24
        P = H * W
        l0 = torch.randn(B * P, 1, H, W, device=_dev())
        pyramid = [p.detach() for p in torch_ref.corr_pyramid(l0, 4)]
        coords = (torch.rand(B, 2, H, W, device=_dev()) *
                  torch.tensor([W, H], device=_dev()).view(1, 2, 1, 1))

        out = CorrLookupFn.apply(coords, radius, *pyramid)[0]
        ref = torch_ref.corr_lookup(pyramid, coords, radius)
        assert out.shape == ref.shape
        torch.testing.assert_close(out, ref, atol=1e-4, rtol=1e-4)

    def test_backward_matches_ref(self):
        from flowhip.ops import torch_ref
        from flowhip.ops.functional import CorrLookupFn
        torch.manual_seed(5)
        B, H, W, radius = 1, 16, 24, 4  # all 4 levels >= 2px (ref-path
        # bilinear_sampler is singular at 1px levels — see test_models note)
        P = H * W
        l0 = torch.randn(B * P, 1, H, W, device=_dev(), requires_grad=True)
        pyramid = torch_ref.corr_pyramid(l0, 4)
        coords = (torch.rand(B, 2, H, W, device=_dev()) *
                  torch.tensor([W, H], device=_dev()).view(1, 2, 1, 1))

        out = CorrLookupFn.apply(coords, radius, *pyramid)[0]
        g = torch.randn_like(out)
        (dl0,) = torch.autograd.grad(out, l0, g)

        l0r = l0.detach().clone().requires_grad_(True)
        pyr_r = torch_ref.corr_pyramid(l0r, 4)
        ref = torch_ref.corr_lookup(pyr_r, coords, radius)
        (dl0r,) = torch.autograd.grad(ref, l0r, g)

        torch.testing.assert_close(dl0, dl0r, atol=1e-3, rtol=1e-3)

    def test_coords_must_be_detached(self):
        from flowhip.ops.functional import CorrLookupFn
        coords = torch.rand(1, 2, 8, 8, device=_dev(), requires_grad=True)
        l0 = torch.randn(64, 1, 8, 8, device=_dev())
        with pytest.raises(AssertionError):
            CorrLookupFn.apply(coords, 4, l0)


class TestCorrBf16Resident:
    """bf16-resident corr volume + pyramid (north star §5.7 / BASELINE
    config 5): the GEMM emits bf16, pyramid/lookup read+write bf16, all
    blends fp32. Tolerances reflect one bf16 rounding of O(1) values."""

    def test_volume_bf16_close_to_fp32(self):
        from flowhip.ops import torch_ref
        from flowhip.ops.functional import CorrVolumeFn
        from flowhip.utils import layout
        torch.manual_seed(41)
        f1 = torch.randn(2, 128, 14, 32, device=_dev())
        f2 = torch.randn(2, 128, 14, 32, device=_dev())
        old = layout.corr_bf16_enabled()
        layout.set_corr_bf16(True)
        try:
            out = CorrVolumeFn.apply(f1, f2)
        finally:
            layout.set_corr_bf16(old)
        assert out.dtype == torch.bfloat16
        ref = torch_ref.corr_volume(f1, f2)
        torch.testing.assert_close(out.float(), ref, atol=8e-2, rtol=8e-2)

    def test_pyramid_and_lookup_bf16(self):
        from flowhip import ops
        from flowhip.ops import torch_ref
        from flowhip.ops.functional import CorrLookupFn, CorrPyramidFn
        torch.manual_seed(42)
        B, H, W = 1, 16, 24
        P = H * W
        l0f = torch.randn(B * P, 1, H, W, device=_dev())
        l0 = l0f.to(torch.bfloat16).requires_grad_(True)
        pyr = list(CorrPyramidFn.apply(l0, 4))
        assert all(p.dtype == torch.bfloat16 for p in pyr)
        ref_pyr = torch_ref.corr_pyramid(l0.detach().float(), 4)
        for p, r in zip(pyr, ref_pyr):
            torch.testing.assert_close(p.float(), r, atol=2e-2, rtol=2e-2)

        coords = (torch.rand(B, 2, H, W, device=_dev()) *
                  torch.tensor([W, H], device=_dev()).view(1, 2, 1, 1))
        out = CorrLookupFn.apply(coords, 4, *[p.detach().requires_grad_(True)
                                              for p in pyr])[0]
        # lookup output dtype follows the pyramid residency dtype
        assert out.dtype == torch.bfloat16
        ref = torch_ref.corr_lookup([r for r in ref_pyr], coords, 4)
        torch.testing.assert_close(out.float(), ref, atol=3e-2, rtol=3e-2)

    def test_lookup_bwd_bf16_levels(self):
        from flowhip.ops import torch_ref
        from flowhip.ops.functional import CorrLookupFn
        torch.manual_seed(43)
        B, H, W, radius = 1, 16, 24, 4
        P = H * W
        l0f = torch.randn(B * P, 1, H, W, device=_dev())
        pyr_f = [p.detach() for p in torch_ref.corr_pyramid(l0f, 4)]
        pyr_b = [p.to(torch.bfloat16).requires_grad_(True) for p in pyr_f]
        coords = (torch.rand(B, 2, H, W, device=_dev()) *
                  torch.tensor([W, H], device=_dev()).view(1, 2, 1, 1))
        out = CorrLookupFn.apply(coords, radius, *pyr_b)[0]
        g = torch.randn_like(out)
        grads = torch.autograd.grad(out, pyr_b, g)
        pyr_r = [p.detach().float().requires_grad_(True) for p in pyr_b]
        ref = torch_ref.corr_lookup(pyr_r, coords, radius)
        refg = torch.autograd.grad(ref, pyr_r, g.float())
        for d, r in zip(grads, refg):
            assert d.dtype == torch.bfloat16
            torch.testing.assert_close(d.float(), r, atol=5e-2, rtol=5e-2)

    def test_model_bf16_corr_deviation_bounded(self):
        """Full raft_nc_dbl forward: bf16-resident corr vs fp32-resident —
        the EPE-parity ablation VERDICT r01 asks for, in miniature: flow
        outputs must agree within a small fraction of a pixel."""
        from flowhip.config.args import default_ncup_args
        from flowhip.models import build_model
        from flowhip.utils import layout
        torch.manual_seed(44)
        args = default_ncup_args(model="raft_nc_dbl", mixed_precision=True,
                                 dataset="sintel")
        model = build_model(args).to(_dev()).eval()
        layout.apply_channels_last(model)
        img1 = torch.rand(1, 3, 128, 256, device=_dev()) * 255
        img2 = torch.rand(1, 3, 128, 256, device=_dev()) * 255
        outs = {}
        old = layout.corr_bf16_enabled()
        try:
            for mode in (False, True):
                layout.set_corr_bf16(mode)
                with torch.no_grad():
                    _, flow = model(img1, img2, iters=6, test_mode=True)
                outs[mode] = flow.float()
        finally:
            layout.set_corr_bf16(old)
        diff = (outs[True] - outs[False]).norm(dim=1)
        assert torch.isfinite(outs[True]).all()
        # sub-0.1px deviation against the fp32-resident pyramid
        assert diff.mean().item() < 0.1, diff.mean().item()


class TestModelGPU:
    def test_raft_nc_dbl_train_step(self):
        from flowhip import ops
        from flowhip.config.args import default_ncup_args
        from flowhip.models import build_model

        torch.manual_seed(1234)
        args = default_ncup_args(model="raft_nc_dbl", mixed_precision=True)
        model = build_model(args).to(_dev())
        model.train()
        model.freeze_bn()

        h, w = 128, 256
        img1 = torch.rand(2, 3, h, w, device=_dev()) * 255
        img2 = torch.rand(2, 3, h, w, device=_dev()) * 255
        flow_gt = torch.randn(2, 2, h, w, device=_dev())
        valid = torch.ones(2, h, w, device=_dev())

        preds = model(img1, img2, iters=3)
        loss, metrics = ops.sequence_loss(preds, flow_gt, valid, 0.85)
        loss.backward()
        torch.cuda.synchronize()
        assert torch.isfinite(loss).item()
        for n, p in model.named_parameters():
            if p.requires_grad:
                assert p.grad is not None and torch.isfinite(p.grad).all(), n

    @pytest.mark.timeout(900)
    @pytest.mark.parametrize("h,w", [(448, 1024), (456, 1016)])
    def test_flagship_shape_hip_vs_ref(self, h, w):
        """Full train step at the FLAGSHIP shape (and an odd-H8/W8
        alignment-hostile one): HIP-path outputs vs FLOWHIP_FORCE_REF=1
        torch path with shared weights — catches OOB-tail bugs that only
        appear at real tile boundaries."""
        import os

        from flowhip import ops
        from flowhip.config.args import default_ncup_args
        from flowhip.models import build_model
        from flowhip.utils import layout

        torch.manual_seed(1234)
        args = default_ncup_args(model="raft_nc_dbl", mixed_precision=True,
                                 dataset="sintel")
        model = build_model(args).to(_dev())
        model.train()
        model.freeze_bn()

        g = torch.Generator().manual_seed(5)
        img1 = (torch.rand(1, 3, h, w, generator=g) * 255).to(_dev())
        img2 = (torch.rand(1, 3, h, w, generator=g) * 255).to(_dev())
        flow_gt = torch.randn(1, 2, h, w, generator=g).to(_dev())
        valid = torch.ones(1, h, w, device=_dev())

        def run(force_ref):
            old_env = os.environ.get("FLOWHIP_FORCE_REF")
            old_bf = layout.corr_bf16_enabled()
            layout.set_corr_bf16(False)  # same-resolution comparison
            if force_ref:
                os.environ["FLOWHIP_FORCE_REF"] = "1"
            try:
                model.zero_grad(set_to_none=True)
                if force_ref:
                    i1, i2 = img1.contiguous(), img2.contiguous()
                else:
                    layout.apply_channels_last(model)
                    i1 = layout.to_model_layout(img1)
                    i2 = layout.to_model_layout(img2)
                preds = model(i1, i2, iters=12)
                loss, metrics = ops.sequence_loss(preds, flow_gt, valid, 0.85)
                loss.backward()
                torch.cuda.synchronize()
                return (loss.item(), metrics["epe"],
                        preds[-1].detach().float())
            finally:
                layout.set_corr_bf16(old_bf)
                if force_ref:
                    if old_env is None:
                        os.environ.pop("FLOWHIP_FORCE_REF", None)
                    else:
                        os.environ["FLOWHIP_FORCE_REF"] = old_env

        loss_h, epe_h, flow_h = run(force_ref=False)
        loss_r, epe_r, flow_r = run(force_ref=True)
        assert torch.isfinite(flow_h).all()
        # both paths run bf16 autocast; differences come from MFMA-vs-MIOpen
        # kernel numerics amplified over 12 refinement iterations
        assert abs(loss_h - loss_r) < 0.05 * max(1.0, abs(loss_r)), \
            (loss_h, loss_r)
        assert abs(epe_h - epe_r) < 0.05 * max(1.0, epe_r), (epe_h, epe_r)
        # the flow FIELD drifts smoothly as per-kernel rounding (different
        # MFMA k-orders vs MIOpen) iterates 12x on a random-init model;
        # an indexing/OOB bug shows as gross garbage, not sub-pixel drift
        diff = (flow_h - flow_r).norm(dim=1)
        mag = flow_r.norm(dim=1).mean().item()
        assert diff.mean().item() < max(0.5, 0.05 * mag), \
            (diff.mean().item(), mag)
        assert diff.max().item() < max(5.0, 0.5 * mag), \
            (diff.max().item(), mag)

    def test_gpu_matches_cpu_forward(self):
        """Same weights + inputs: GPU (HIP kernels, fp32 autocast off) vs CPU
        reference path agree within bf16-corr tolerance."""
        from flowhip.config.args import default_ncup_args
        from flowhip.models import build_model

        torch.manual_seed(1234)
        args = default_ncup_args(model="raft_nc_dbl", mixed_precision=False)
        model = build_model(args)
        model.eval()

        img1 = torch.rand(1, 3, 128, 128) * 255
        img2 = torch.rand(1, 3, 128, 128) * 255

        with torch.no_grad():
            low_cpu, up_cpu = model(img1, img2, iters=2, test_mode=True)
            model_gpu = model.to(_dev())
            low_gpu, up_gpu = model_gpu(img1.to(_dev()), img2.to(_dev()),
                                        iters=2, test_mode=True)

        torch.testing.assert_close(low_gpu.cpu(), low_cpu, atol=0.05, rtol=0.05)
        torch.testing.assert_close(up_gpu.cpu(), up_cpu, atol=0.5, rtol=0.1)


class TestConvexUpsample:
    def test_forward_matches_ref(self):
        from flowhip.ops import torch_ref
        from flowhip.ops.functional_upsample import ConvexUpsampleFn
        torch.manual_seed(6)
        flow = torch.randn(2, 2, 12, 16, device=_dev())
        mask = torch.randn(2, 576, 12, 16, device=_dev())
        out = ConvexUpsampleFn.apply(flow, mask, 8)
        ref = torch_ref.convex_upsample(flow, mask, 8)
        torch.testing.assert_close(out, ref, atol=1e-4, rtol=1e-4)

    def test_backward_matches_ref(self):
        from flowhip.ops import torch_ref
        from flowhip.ops.functional_upsample import ConvexUpsampleFn
        torch.manual_seed(7)
        flow = torch.randn(1, 2, 8, 12, device=_dev(), requires_grad=True)
        mask = torch.randn(1, 576, 8, 12, device=_dev(), requires_grad=True)
        g = torch.randn(1, 2, 64, 96, device=_dev())

        out = ConvexUpsampleFn.apply(flow, mask, 8)
        df, dm = torch.autograd.grad(out, (flow, mask), g)

        fr = flow.detach().clone().requires_grad_(True)
        mr = mask.detach().clone().requires_grad_(True)
        ref = torch_ref.convex_upsample(fr, mr, 8)
        rf, rm = torch.autograd.grad(ref, (fr, mr), g)

        torch.testing.assert_close(df, rf, atol=1e-3, rtol=1e-3)
        torch.testing.assert_close(dm, rm, atol=1e-3, rtol=1e-3)


class TestNConv:
    @pytest.mark.parametrize("ci,co,k,bias", [(1, 2, 5, False), (2, 2, 5, False),
                                              (4, 2, 3, False), (2, 1, 1, False),
                                              (2, 2, 3, True)])
    def test_forward_matches_ref(self, ci, co, k, bias):
        from flowhip.ops import torch_ref
        from flowhip.ops.functional_nconv import NConv2dFn
        torch.manual_seed(8)
        data = torch.randn(3, ci, 24, 20, device=_dev())
        conf = torch.rand(3, ci, 24, 20, device=_dev())
        weight = torch.rand(co, ci, k, k, device=_dev()) + 0.05
        b = torch.randn(co, device=_dev()) if bias else None

        out, cout = NConv2dFn.apply(data, conf, weight, b, k // 2, 1e-20, True)
        rout, rcout = torch_ref.nconv2d(data, conf, weight, b, 1, k // 2)
        torch.testing.assert_close(out, rout, atol=1e-4, rtol=1e-4)
        torch.testing.assert_close(cout, rcout, atol=1e-4, rtol=1e-4)

    def test_backward_matches_ref(self):
        from flowhip.ops import torch_ref
        from flowhip.ops.functional_nconv import NConv2dFn
        torch.manual_seed(9)
        data = torch.randn(2, 1, 16, 20, device=_dev(), requires_grad=True)
        conf = torch.rand(2, 1, 16, 20, device=_dev(), requires_grad=True)
        weight = (torch.rand(2, 1, 5, 5, device=_dev()) + 0.05).requires_grad_(True)

        out, cout = NConv2dFn.apply(data, conf, weight, None, 2, 1e-20, True)
        g1 = torch.randn_like(out)
        g2 = torch.randn_like(cout)
        dd, dc, dw = torch.autograd.grad((out, cout), (data, conf, weight),
                                         (g1, g2))

        dr = data.detach().clone().requires_grad_(True)
        cr = conf.detach().clone().requires_grad_(True)
        wr = weight.detach().clone().requires_grad_(True)
        rout, rcout = torch_ref.nconv2d(dr, cr, wr, None, 1, 2)
        rd, rc, rw = torch.autograd.grad((rout, rcout), (dr, cr, wr), (g1, g2))

        torch.testing.assert_close(dd, rd, atol=1e-3, rtol=1e-3)
        torch.testing.assert_close(dc, rc, atol=1e-3, rtol=1e-3)
        torch.testing.assert_close(dw, rw, atol=1e-3, rtol=1e-3)

    def test_unet_gpu_matches_ref_path(self):
        """Whole NConvUNet (shipped config) on GPU HIP path vs forced-ref."""
        import os
        from flowhip.nn.nconv import NConvUNet
        torch.manual_seed(10)
        net = NConvUNet(in_ch=1, channels_multiplier=2, num_downsampling=1,
                        encoder_filter_sz=5, decoder_filter_sz=3,
                        out_filter_sz=1, use_bias=False,
                        data_pooling="conf_based", shared_encoder=True,
                        use_double_conv=False).to(_dev())
        data = torch.randn(4, 1, 64, 64, device=_dev())
        conf = torch.rand(4, 1, 64, 64, device=_dev())
        out, cout = net((data, conf))

        os.environ["FLOWHIP_FORCE_REF"] = "1"
        try:
            rout, rcout = net((data, conf))
        finally:
            del os.environ["FLOWHIP_FORCE_REF"]
        torch.testing.assert_close(out, rout, atol=1e-4, rtol=1e-4)
        torch.testing.assert_close(cout, rcout, atol=1e-4, rtol=1e-4)


class TestHipGraph:
    def test_graphed_inference_matches_eager(self):
        from flowhip.config.args import default_ncup_args
        from flowhip.engine.graph import GraphedInference
        from flowhip.models import build_model

        torch.manual_seed(1234)
        args = default_ncup_args(model="raft_nc_dbl", mixed_precision=True)
        model = build_model(args).to(_dev()).eval()

        shape = (1, 3, 128, 256)
        img1 = torch.rand(shape, device=_dev()) * 255
        img2 = torch.rand(shape, device=_dev()) * 255

        with torch.no_grad():
            low_e, up_e = model(img1, img2, iters=4, test_mode=True)
        g = GraphedInference(model, shape, iters=4)
        low_g, up_g = g(img1, img2)

        # iterative refinement amplifies tiny numeric differences from
        # capture-context kernel selection; require agreement at the level
        # eager-vs-eager nondeterminism would allow (flow magnitudes O(10))
        torch.testing.assert_close(low_g, low_e, atol=0.05, rtol=0.05)
        torch.testing.assert_close(up_g, up_e, atol=0.4, rtol=0.1)

        # replay with different inputs must track eager
        img3 = torch.rand(shape, device=_dev()) * 255
        with torch.no_grad():
            low_e2, up_e2 = model(img3, img2, iters=4, test_mode=True)
        low_g2, up_g2 = g(img3, img2)
        torch.testing.assert_close(up_g2, up_e2, atol=0.4, rtol=0.1)


class TestCorrPyramidFused:
    def test_forward_matches_avgpool_chain(self):
        from flowhip import ops
        from flowhip.ops import torch_ref
        torch.manual_seed(5)
        for (h, w) in [(56, 128), (23, 31), (36, 120)]:
            corr = torch.randn(64, 1, h, w, device=_dev())
            got = ops.corr_pyramid(corr, 4)
            ref = torch_ref.corr_pyramid(corr.cpu(), 4)
            assert len(got) == len(ref)
            for g, r in zip(got, ref):
                torch.testing.assert_close(g.cpu(), r, atol=1e-6, rtol=1e-6)

    def test_kitti_submission_shape_stays_on_hip(self):
        """47x156 (KITTI full-res 375x1242 / 8) exceeded round-1's static
        56x128 LDS cap and silently fell back to torch; the dynamic-LDS
        kernel must take it."""
        import flowhip._C as C
        from flowhip import ops
        from flowhip.ops import torch_ref
        assert C.corr_pyramid_fits(47, 156, False)
        assert C.corr_pyramid_fits(47, 156, True)
        torch.manual_seed(51)
        corr = torch.randn(32, 1, 47, 156, device=_dev())
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("error")  # fallback warns -> fail
            got = ops.corr_pyramid(corr, 4)
        ref = torch_ref.corr_pyramid(corr.cpu(), 4)
        for g, r in zip(got, ref):
            torch.testing.assert_close(g.cpu(), r, atol=1e-6, rtol=1e-6)

    def test_backward_matches_autograd(self):
        from flowhip import ops
        from flowhip.ops import torch_ref
        torch.manual_seed(6)
        corr = torch.randn(16, 1, 24, 40, device=_dev(), requires_grad=True)
        corr_cpu = corr.detach().cpu().requires_grad_(True)
        levels = ops.corr_pyramid(corr, 4)
        ref_levels = torch_ref.corr_pyramid(corr_cpu, 4)
        gs = [torch.randn_like(l) for l in levels]
        torch.autograd.backward(levels, gs)
        torch.autograd.backward(ref_levels, [g.cpu() for g in gs])
        torch.testing.assert_close(corr.grad.cpu(), corr_cpu.grad,
                                   atol=1e-5, rtol=1e-5)


class TestPacPool:
    @pytest.mark.parametrize("kch,stride", [(1, 1), (1, 2), (0, 1)])
    def test_matches_unfold_ref(self, kch, stride):
        """HIP pacpool vs the unfold composition (reference
        pac_modules.py:288-329); kch 0 means per-channel kernels."""
        from flowhip.nn.pac import nd2col, pacpool2d
        torch.manual_seed(71)
        B, C, H, W, K = 2, 4, 18, 22, 3
        pad = K // 2
        OH = (H + 2 * pad - K) // stride + 1
        OW = (W + 2 * pad - K) // stride + 1
        x = torch.randn(B, C, H, W, device=_dev(), requires_grad=True)
        ch = 1 if kch == 1 else C
        kr = torch.rand(B, ch, K, K, OH, OW, device=_dev(),
                        requires_grad=True)

        out = pacpool2d(x, kr, K, stride=stride, padding=pad)
        x2 = x.detach().clone().requires_grad_(True)
        k2 = kr.detach().clone().requires_grad_(True)
        cols = nd2col(x2, (K, K), stride=stride, padding=pad)
        ref = (cols * k2).view(B, C, -1, OH, OW).sum(dim=2)
        torch.testing.assert_close(out, ref, atol=1e-4, rtol=1e-4)

        g = torch.randn_like(ref)
        out.backward(g)
        ref.backward(g)
        torch.testing.assert_close(x.grad, x2.grad, atol=1e-4, rtol=1e-4)
        torch.testing.assert_close(kr.grad, k2.grad, atol=1e-4, rtol=1e-4)


class TestFrozenBatchNorm:
    def test_col_sum2_matches_torch(self):
        import flowhip._C as C
        torch.manual_seed(61)
        for (m, c) in [(3 * 24 * 40, 64), (1111, 96), (256, 8)]:
            g = torch.randn(1, c, 1, m, device=_dev()).to(torch.bfloat16) \
                .contiguous(memory_format=torch.channels_last)
            x = torch.randn(1, c, 1, m, device=_dev()).to(torch.bfloat16) \
                .contiguous(memory_format=torch.channels_last)
            out = C.col_sum2_bf16(g, x)
            gf, xf = g.float(), x.float()
            ref0 = gf.sum(dim=(0, 2, 3))
            ref1 = (gf * xf).sum(dim=(0, 2, 3))
            torch.testing.assert_close(out[0], ref0, atol=2e-1, rtol=1e-2)
            torch.testing.assert_close(out[1], ref1, atol=5e-1, rtol=2e-2)

    def test_plane_sum_nchw(self):
        import flowhip._C as C
        torch.manual_seed(63)
        for (b, c, h, w) in [(4, 2, 30, 44), (2, 3, 23, 31), (1, 8, 64, 64)]:
            x = torch.randn(b, c, h, w, device=_dev())
            y = torch.randn(b, c, h, w, device=_dev())
            torch.testing.assert_close(C.plane_sum_nchw(x),
                                       x.sum(dim=(0, 2, 3)),
                                       atol=1e-3, rtol=1e-4)
            torch.testing.assert_close(C.plane_sum_nchw(x, y),
                                       (x * y).sum(dim=(0, 2, 3)),
                                       atol=1e-3, rtol=1e-4)

    def test_frozen_bn_matches_stock_eval_bn(self):
        from flowhip.nn.norm import BatchNorm2d
        torch.manual_seed(62)
        bn = BatchNorm2d(64).to(_dev())
        ref = torch.nn.BatchNorm2d(64).to(_dev())
        with torch.no_grad():
            bn.weight.copy_(torch.rand(64) + 0.5)
            bn.bias.copy_(torch.randn(64))
            bn.running_mean.copy_(torch.randn(64))
            bn.running_var.copy_(torch.rand(64) + 0.3)
        ref.load_state_dict(bn.state_dict())
        bn.eval()
        ref.eval()

        x = torch.randn(2, 64, 24, 40, device=_dev()).to(torch.bfloat16) \
            .contiguous(memory_format=torch.channels_last) \
            .requires_grad_(True)
        x2 = x.detach().float().requires_grad_(True)
        y = bn(x)
        yr = ref(x2)
        assert y.dtype == torch.bfloat16
        torch.testing.assert_close(y.float(), yr, atol=5e-2, rtol=5e-2)

        g = torch.randn_like(yr)
        y.backward(g.to(torch.bfloat16)
                   .contiguous(memory_format=torch.channels_last))
        yr.backward(g)
        torch.testing.assert_close(x.grad.float(), x2.grad,
                                   atol=5e-2, rtol=5e-2)
        torch.testing.assert_close(bn.weight.grad, ref.weight.grad,
                                   atol=2.0, rtol=2e-2)
        torch.testing.assert_close(bn.bias.grad, ref.bias.grad,
                                   atol=1.0, rtol=2e-2)

    def test_frozen_bn_training_mode_uses_stock(self):
        from flowhip.nn.norm import BatchNorm2d
        bn = BatchNorm2d(16).to(_dev()).train()
        x = torch.randn(2, 16, 8, 8, device=_dev()) \
            .contiguous(memory_format=torch.channels_last)
        y = bn(x)  # batch-stats path (chairs stage)
        ref = torch.nn.functional.batch_norm(
            x, None, None, bn.weight, bn.bias, True, 0.1, bn.eps)
        torch.testing.assert_close(y, ref, atol=1e-5, rtol=1e-5)


class TestSequenceLossFused:
    def test_matches_torch_ref(self):
        from flowhip import ops
        from flowhip.ops import torch_ref
        torch.manual_seed(7)
        B, H, W, n = 2, 64, 96, 5
        preds = [torch.randn(B, 2, H, W, device=_dev(), requires_grad=True)
                 for _ in range(n)]
        gt = torch.randn(B, 2, H, W, device=_dev()) * 30
        gt[0, :, :8, :8] = 500.0  # exercise the max-flow exclusion
        valid = (torch.rand(B, H, W, device=_dev()) > 0.2).float()

        loss, metrics = ops.sequence_loss(preds, gt, valid, gamma=0.85)
        preds_cpu = [p.detach().cpu().requires_grad_(True) for p in preds]
        ref_loss, ref_metrics = torch_ref.sequence_loss(
            preds_cpu, gt.cpu(), valid.cpu(), gamma=0.85)

        assert loss.item() == pytest.approx(ref_loss.item(), rel=1e-4)
        for k in ("epe", "1px", "3px", "5px"):
            assert metrics[k] == pytest.approx(ref_metrics[k], rel=1e-4,
                                               abs=1e-6)

        loss.backward()
        ref_loss.backward()
        for p, pc in zip(preds, preds_cpu):
            torch.testing.assert_close(p.grad.cpu(), pc.grad,
                                       atol=1e-6, rtol=1e-5)


class TestGruGatesFused:
    @pytest.mark.parametrize("dtype,cl", [
        (torch.float32, False), (torch.float32, True),
        (torch.bfloat16, True)])
    def test_matches_torch_math(self, dtype, cl):
        from flowhip.ops.functional_gru import GruGate1Fn, GruGate2Fn
        torch.manual_seed(11)
        B, C, H, W = 2, 32, 14, 18
        mf = torch.channels_last if cl else torch.contiguous_format

        def mk(c, grad=True):
            t = torch.randn(B, c, H, W, device=_dev()).to(dtype) \
                .contiguous(memory_format=mf)
            return t.requires_grad_(grad)

        zr, h, qp = mk(2 * C), mk(C), mk(C)
        z, rh = GruGate1Fn.apply(zr, h)
        hnew = GruGate2Fn.apply(qp, z, h)

        zr2 = zr.detach().float().requires_grad_(True)
        h2 = h.detach().float().requires_grad_(True)
        qp2 = qp.detach().float().requires_grad_(True)
        z2, r2 = torch.sigmoid(zr2).chunk(2, dim=1)
        hnew2 = (1 - z2) * h2 + z2 * torch.tanh(qp2)

        tol = dict(atol=1e-5, rtol=1e-5) if dtype == torch.float32 else \
            dict(atol=2e-2, rtol=2e-2)
        torch.testing.assert_close(hnew.float(), hnew2, **tol)
        torch.testing.assert_close(rh.float(), (r2 * h2), **tol)

        g = torch.randn_like(hnew2)
        # route rh's grad too (as convq would): use rh.sum()*0 + hnew path
        (hnew.float() * g).sum().backward()
        (hnew2 * g).sum().backward()
        torch.testing.assert_close(zr.grad.float(), zr2.grad, **tol)
        torch.testing.assert_close(qp.grad.float(), qp2.grad, **tol)
        torch.testing.assert_close(h.grad.float(), h2.grad, **tol)


class TestInstanceNormCL:
    @pytest.mark.parametrize("dtype,C", [(torch.float32, 64),
                                         (torch.float32, 96),
                                         (torch.bfloat16, 128)])
    def test_matches_torch(self, dtype, C):
        from flowhip.nn.norm import InstanceNorm2d
        torch.manual_seed(13)
        x = torch.randn(3, C, 20, 34, device=_dev()).to(dtype) \
            .contiguous(memory_format=torch.channels_last).requires_grad_(True)
        m = InstanceNorm2d(C).to(_dev())
        y = m(x)

        x2 = x.detach().float().requires_grad_(True)
        y2 = torch.nn.functional.instance_norm(x2, eps=m.eps)

        tol = dict(atol=1e-5, rtol=1e-5) if dtype == torch.float32 else \
            dict(atol=3e-2, rtol=3e-2)
        torch.testing.assert_close(y.float(), y2, **tol)

        g = torch.randn_like(y2)
        (y.float() * g).sum().backward()
        (y2 * g).sum().backward()
        torch.testing.assert_close(x.grad.float(), x2.grad, **tol)


class TestZeroInjectHIP:
    def test_matches_torch_ref(self):
        from flowhip import ops
        from flowhip.ops import torch_ref
        torch.manual_seed(14)
        x = torch.randn(4, 2, 112, 256, device=_dev(), requires_grad=True)
        out = ops.zero_inject(x, 4, 4)
        x2 = x.detach().cpu().requires_grad_(True)
        ref = torch_ref.zero_inject(x2, 4, 4)
        torch.testing.assert_close(out.cpu(), ref)
        g = torch.randn_like(ref)
        (out * g.to(_dev())).sum().backward()
        (ref * g).sum().backward()
        torch.testing.assert_close(x.grad.cpu(), x2.grad)


class TestConvGemm:
    SHAPES = [
        # (Cin, Cout, KH, KW) — the update-block inventory (update.py:6-146)
        (324, 256, 1, 1),   # convc1 (Cin % 8 != 0: zero-weight tail path)
        (256, 192, 3, 3),   # convc2
        (2, 128, 7, 7),     # convf1 (tiny Cin)
        (128, 64, 3, 3),    # convf2
        (256, 126, 3, 3),   # conv (ragged Cout)
        (384, 256, 1, 5),   # packed zr horizontal
        (384, 128, 5, 1),   # q vertical
        (256, 2, 3, 3),     # flow head out (Cout=2)
    ]

    @pytest.mark.parametrize("ci,co,kh,kw", SHAPES)
    def test_fwd_bwd_matches_miopen(self, ci, co, kh, kw):
        from flowhip.ops.functional_conv import fused_conv2d, can_fuse_conv
        torch.manual_seed(17)
        B, H, W = 2, 24, 40
        x = (torch.randn(B, ci, H, W, device=_dev()) / 8).to(torch.bfloat16) \
            .contiguous(memory_format=torch.channels_last).requires_grad_(True)
        w = (torch.randn(co, ci, kh, kw, device=_dev()) /
             (ci * kh * kw) ** 0.5).requires_grad_(True)
        b = torch.randn(co, device=_dev()).requires_grad_(True)
        pad = (kh // 2, kw // 2)
        assert can_fuse_conv(x, w, 1, pad, 1, 1)

        cache = {}
        out = fused_conv2d(x, w, b, 1, pad, 1, 1, cache)
        ref = torch.nn.functional.conv2d(
            x.detach().float(), w.detach().float(), b.detach().float(),
            padding=pad)
        tol = dict(atol=5e-2, rtol=5e-2)  # bf16 inputs, fp32 accumulate
        torch.testing.assert_close(out.float(), ref, **tol)

        g = torch.randn_like(ref).to(torch.bfloat16) \
            .contiguous(memory_format=torch.channels_last)
        out.backward(g)
        x2 = x.detach().float().requires_grad_(True)
        w2 = w.detach().float().requires_grad_(True)
        b2 = b.detach().float().requires_grad_(True)
        torch.nn.functional.conv2d(x2, w2, b2, padding=pad).backward(
            g.float())
        torch.testing.assert_close(x.grad.float(), x2.grad, **tol)
        torch.testing.assert_close(w.grad.float(), w2.grad,
                                   atol=1e-1, rtol=5e-2)
        torch.testing.assert_close(b.grad.float(), b2.grad,
                                   atol=1e-1, rtol=5e-2)

    STRIDED = [
        # (Cin, Cout, K, stride, H, W) — encoder inventory (extractor.py):
        # 7x7 s2 stem (3ch zero-pad path), stage-transition 3x3 s2,
        # downsample 1x1 s2; odd/hostile dims too
        (3, 64, 7, 2, 30, 48),
        (64, 96, 3, 2, 24, 40),
        (96, 128, 3, 2, 23, 37),
        (64, 96, 1, 2, 24, 40),
        (96, 96, 3, 1, 24, 40),
    ]

    @pytest.mark.parametrize("ci,co,k,s,H,W", STRIDED)
    def test_strided_fwd_bwd_matches_torch(self, ci, co, k, s, H, W):
        """Strided direct conv (smode 1) + its transposed backward-data
        (smode 2) + strided wrw vs the fp32 torch oracle."""
        from flowhip.ops.functional_conv import fused_conv2d, can_fuse_conv
        torch.manual_seed(23)
        B = 2
        x = (torch.randn(B, ci, H, W, device=_dev()) / 8).to(torch.bfloat16) \
            .contiguous(memory_format=torch.channels_last).requires_grad_(True)
        w = (torch.randn(co, ci, k, k, device=_dev()) /
             (ci * k * k) ** 0.5).requires_grad_(True)
        b = torch.randn(co, device=_dev()).requires_grad_(True)
        pad = k // 2
        assert can_fuse_conv(x, w, s, pad, 1, 1)

        out = fused_conv2d(x, w, b, s, pad, 1, 1, {})
        ref = torch.nn.functional.conv2d(
            x.detach().float(), w.detach().float(), b.detach().float(),
            stride=s, padding=pad)
        tol = dict(atol=5e-2, rtol=5e-2)
        torch.testing.assert_close(out.float(), ref, **tol)

        g = torch.randn_like(ref).to(torch.bfloat16) \
            .contiguous(memory_format=torch.channels_last)
        out.backward(g)
        x2 = x.detach().float().requires_grad_(True)
        w2 = w.detach().float().requires_grad_(True)
        b2 = b.detach().float().requires_grad_(True)
        torch.nn.functional.conv2d(x2, w2, b2, stride=s,
                                   padding=pad).backward(g.float())
        torch.testing.assert_close(x.grad.float(), x2.grad, **tol)
        torch.testing.assert_close(w.grad.float(), w2.grad,
                                   atol=1e-1, rtol=5e-2)
        torch.testing.assert_close(b.grad.float(), b2.grad,
                                   atol=1e-1, rtol=5e-2)

    def test_large_m_bm128_tile(self):
        """Encoder-sized M routes to the BM=128 8-wave tile (the launcher
        switches at >=320 tiles); oracle-check fwd + both backwards there,
        including a non-128-aligned M tail."""
        from flowhip.ops.functional_conv import fused_conv2d
        torch.manual_seed(29)
        B, ci, co, H, W = 2, 64, 64, 161, 161  # M = 51842 -> 406 tiles
        x = (torch.randn(B, ci, H, W, device=_dev()) / 8).to(torch.bfloat16) \
            .contiguous(memory_format=torch.channels_last).requires_grad_(True)
        w = (torch.randn(co, ci, 3, 3, device=_dev()) / 24).requires_grad_(True)
        out = fused_conv2d(x, w, None, 1, 1, 1, 1, {})
        ref = torch.nn.functional.conv2d(x.detach().float(),
                                         w.detach().float(), padding=1)
        tol = dict(atol=5e-2, rtol=5e-2)
        torch.testing.assert_close(out.float(), ref, **tol)
        g = torch.randn_like(ref).to(torch.bfloat16) \
            .contiguous(memory_format=torch.channels_last)
        out.backward(g)
        x2 = x.detach().float().requires_grad_(True)
        w2 = w.detach().float().requires_grad_(True)
        torch.nn.functional.conv2d(x2, w2, padding=1).backward(g.float())
        torch.testing.assert_close(x.grad.float(), x2.grad, **tol)
        torch.testing.assert_close(w.grad.float(), w2.grad,
                                   atol=2e-1, rtol=5e-2)

    @pytest.mark.parametrize("ci,co,kh,kw", [
        (96, 64, 3, 3), (64, 96, 3, 3), (128, 126, 3, 3),
        (128, 128, 1, 5), (128, 64, 5, 1),
    ])
    def test_halo_path_matches_torch(self, ci, co, kh, kw):
        """Stride-1 3x3 / 1x5 / 5x1 at grid sizes that take the
        halo-staged kernel (>=320 workgroups), with ragged Cin/Cout and
        edge tiles."""
        from flowhip.ops.functional_conv import fused_conv2d
        torch.manual_seed(37)
        B, H, W = 3, 126, 130  # ragged in both tile dims
        pad = (kh // 2, kw // 2)
        x = (torch.randn(B, ci, H, W, device=_dev()) / 8).to(torch.bfloat16) \
            .contiguous(memory_format=torch.channels_last).requires_grad_(True)
        w = (torch.randn(co, ci, kh, kw, device=_dev()) /
             (ci * kh * kw) ** 0.5).requires_grad_(True)
        b = torch.randn(co, device=_dev()).requires_grad_(True)
        out = fused_conv2d(x, w, b, 1, pad, 1, 1, {})
        ref = torch.nn.functional.conv2d(
            x.detach().float(), w.detach().float(), b.detach().float(),
            padding=pad)
        tol = dict(atol=5e-2, rtol=5e-2)
        torch.testing.assert_close(out.float(), ref, **tol)
        g = torch.randn_like(ref).to(torch.bfloat16) \
            .contiguous(memory_format=torch.channels_last)
        out.backward(g)
        x2 = x.detach().float().requires_grad_(True)
        w2 = w.detach().float().requires_grad_(True)
        b2 = b.detach().float().requires_grad_(True)
        torch.nn.functional.conv2d(x2, w2, b2, padding=pad).backward(
            g.float())
        torch.testing.assert_close(x.grad.float(), x2.grad, **tol)
        torch.testing.assert_close(w.grad.float(), w2.grad,
                                   atol=2e-1, rtol=5e-2)

    def test_fused_encoder_matches_miopen_encoder(self):
        """BasicEncoder with FLOWHIP_FUSED_ENCODER=1 (fused stride-1 AND
        stride-2 convs) vs the MIOpen path, same weights."""
        import importlib
        import os
        from flowhip.nn import extractor as ex
        torch.manual_seed(31)
        old = os.environ.get("FLOWHIP_FUSED_ENCODER")
        try:
            os.environ["FLOWHIP_FUSED_ENCODER"] = "1"
            enc_f = ex.BasicEncoder(output_dim=128, norm_fn="instance").to(_dev())
            os.environ["FLOWHIP_FUSED_ENCODER"] = "0"
            enc_m = ex.BasicEncoder(output_dim=128, norm_fn="instance").to(_dev())
        finally:
            if old is None:
                os.environ.pop("FLOWHIP_FUSED_ENCODER", None)
            else:
                os.environ["FLOWHIP_FUSED_ENCODER"] = old
        enc_m.load_state_dict(enc_f.state_dict())
        x = torch.randn(2, 3, 128, 160, device=_dev())
        with torch.autocast("cuda", dtype=torch.bfloat16):
            yf = enc_f(x.contiguous(memory_format=torch.channels_last))
            ym = enc_m(x.contiguous(memory_format=torch.channels_last))
        # 8 bf16 convs + instance norms chained amplify per-layer rounding
        # (different k-orders) multiplicatively; anchor both bf16 paths
        # against the fp32 oracle instead of against each other: the MFMA
        # path may not sit materially farther from fp32 than MIOpen does.
        with torch.no_grad():
            y32 = enc_m(x)  # fp32, no autocast
        d_f = (yf.float() - y32).abs().mean().item()
        d_m = (ym.float() - y32).abs().mean().item()
        assert d_f < max(2.0 * d_m, 0.02), (d_f, d_m)

    def test_narrowed_input_view(self):
        # a channel-narrowed channels-last view (the 324-of-328 corr case)
        from flowhip.ops.functional_conv import fused_conv2d
        torch.manual_seed(18)
        B, H, W = 2, 16, 24
        full = (torch.randn(B, 328, H, W, device=_dev()) / 8) \
            .to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        x = full[:, :324]
        w = (torch.randn(64, 324, 1, 1, device=_dev()) / 18)
        out = fused_conv2d(x, w, None, 1, 0, 1, 1, {})
        ref = torch.nn.functional.conv2d(x.float(), w.float())
        torch.testing.assert_close(out.float(), ref, atol=5e-2, rtol=5e-2)


class TestTransposeCast:
    def test_matches_eager(self):
        import flowhip._C as C
        torch.manual_seed(19)
        for (B, M, N) in [(2, 128, 128), (1, 300, 177), (3, 64, 96)]:
            x = torch.randn(B, M, N, device=_dev())
            got = C.transpose_cast_bf16(x)
            ref = x.transpose(1, 2).to(torch.bfloat16).contiguous()
            torch.testing.assert_close(got, ref)


class TestConfPoolFused:
    def test_matches_torch_ref(self):
        from flowhip import ops
        from flowhip.ops import torch_ref
        torch.manual_seed(21)
        data = torch.randn(3, 2, 30, 44, device=_dev(), requires_grad=True)
        conf = torch.rand(3, 2, 30, 44, device=_dev(), requires_grad=True)
        dds, cds = ops.conf_pool(data, conf)
        d2 = data.detach().cpu().requires_grad_(True)
        c2 = conf.detach().cpu().requires_grad_(True)
        rdds, rcds = torch_ref.conf_pool(d2, c2)
        torch.testing.assert_close(dds.cpu(), rdds)
        torch.testing.assert_close(cds.cpu(), rcds)
        g1, g2 = torch.randn_like(rdds), torch.randn_like(rcds)
        (dds * g1.to(_dev()) + cds * g2.to(_dev())).sum().backward()
        (rdds * g1 + rcds * g2).sum().backward()
        torch.testing.assert_close(data.grad.cpu(), d2.grad)
        torch.testing.assert_close(conf.grad.cpu(), c2.grad)


class TestConvGemmCat2:
    def test_matches_cat_conv(self):
        from flowhip.ops.functional_conv import fused_conv2d_cat2
        torch.manual_seed(23)
        B, H, W = 2, 20, 36
        x1 = (torch.randn(B, 128, H, W, device=_dev()) / 8) \
            .to(torch.bfloat16).contiguous(memory_format=torch.channels_last) \
            .requires_grad_(True)
        x2 = (torch.randn(B, 256, H, W, device=_dev()) / 8) \
            .to(torch.bfloat16).contiguous(memory_format=torch.channels_last) \
            .requires_grad_(True)
        w = (torch.randn(256, 384, 1, 5, device=_dev()) / 44).requires_grad_(True)
        b = torch.randn(256, device=_dev()).requires_grad_(True)
        out = fused_conv2d_cat2(x1, x2, w, b, (0, 2), {}, key=(0,))

        x1r = x1.detach().float().requires_grad_(True)
        x2r = x2.detach().float().requires_grad_(True)
        wr = w.detach().clone().requires_grad_(True)
        br = b.detach().clone().requires_grad_(True)
        ref = torch.nn.functional.conv2d(torch.cat([x1r, x2r], 1), wr, br,
                                         padding=(0, 2))
        tol = dict(atol=5e-2, rtol=5e-2)
        torch.testing.assert_close(out.float(), ref, **tol)

        g = torch.randn_like(ref).to(torch.bfloat16) \
            .contiguous(memory_format=torch.channels_last)
        out.backward(g)
        ref.backward(g.float())
        torch.testing.assert_close(x1.grad.float(), x1r.grad, **tol)
        torch.testing.assert_close(x2.grad.float(), x2r.grad, **tol)
        torch.testing.assert_close(w.grad.float(), wr.grad, atol=1e-1,
                                   rtol=5e-2)


class TestGruZrConvNoScope:
    """fused_gru_zr_conv outside a wrw_accumulate_scope (ConvGemmCat2ZrFn:
    cached packed bias, gradients sliced back to the four parameters)
    against fp32 F.conv2d of the same bf16-rounded inputs. h 64 + x 192
    channels -> 2 x 64 gates: 2 x 4 weight-gradient tiles, so dW takes the
    halo-staged path; 9 x 37 leaves tile tails in both directions."""

    @pytest.mark.parametrize("KH,KW", [(1, 5), (5, 1)], ids=["1x5", "5x1"])
    def test_matches_cat_conv(self, KH, KW):
        from flowhip.ops import functional_conv as fc
        torch.manual_seed(29)
        B, H, W, CH, CX, O = 2, 9, 37, 64, 192, 64
        pad = (KH // 2, KW // 2)

        def cl(c):
            return (torch.randn(B, c, H, W, device=_dev()) / 8) \
                .to(torch.bfloat16) \
                .contiguous(memory_format=torch.channels_last) \
                .requires_grad_(True)

        h, x = cl(CH), cl(CX)
        convz = torch.nn.Conv2d(CH + CX, O, (KH, KW), padding=pad).to(_dev())
        convr = torch.nn.Conv2d(CH + CX, O, (KH, KW), padding=pad).to(_dev())
        with torch.no_grad():
            for conv in (convz, convr):
                conv.weight.copy_(torch.randn_like(conv.weight) / 44)
                conv.bias.copy_(torch.randn_like(conv.bias))

        assert getattr(fc._tls, "handles", None) is None  # no scope open
        out = fc.fused_gru_zr_conv(h, x, convz, convr, pad, {})
        assert type(out.grad_fn).__name__ == "ConvGemmCat2ZrFnBackward"

        hr = h.detach().float().requires_grad_(True)
        xr = x.detach().float().requires_grad_(True)
        ref_p = [p.detach().clone().requires_grad_(True) for p in
                 (convz.weight, convr.weight, convz.bias, convr.bias)]
        ref = torch.nn.functional.conv2d(
            torch.cat([hr, xr], 1), torch.cat(ref_p[:2]), torch.cat(ref_p[2:]),
            padding=pad)
        tol = dict(atol=5e-2, rtol=5e-2)
        torch.testing.assert_close(out.float(), ref, **tol)

        g = torch.randn_like(ref).to(torch.bfloat16) \
            .contiguous(memory_format=torch.channels_last)
        out.backward(g)
        ref.backward(g.float())
        torch.testing.assert_close(h.grad.float(), hr.grad, **tol)
        torch.testing.assert_close(x.grad.float(), xr.grad, **tol)
        for p, r in zip((convz.weight, convr.weight, convz.bias, convr.bias),
                        ref_p):
            assert p.grad.shape == r.grad.shape
            torch.testing.assert_close(p.grad.float(), r.grad, atol=1e-1,
                                       rtol=5e-2)


class TestAreaUp2x:
    def test_matches_interpolate(self):
        from flowhip import ops
        torch.manual_seed(25)
        x = torch.randn(2, 8, 14, 22, device=_dev(), requires_grad=True)
        out = ops.area_resize(x, (28, 44))
        x2 = x.detach().cpu().requires_grad_(True)
        ref = torch.nn.functional.interpolate(x2, (28, 44), mode="area")
        torch.testing.assert_close(out.cpu(), ref)
        g = torch.randn_like(ref)
        (out * g.to(_dev())).sum().backward()
        (ref * g).sum().backward()
        torch.testing.assert_close(x.grad.cpu(), x2.grad)


class TestWeightsEstBf16:
    def test_conf_close_to_fp32_oracle(self):
        """The confidence net runs bf16/NHWC on GPU (documented deviation —
        the reference ran it fp32 only because its autocast region ended
        before the upsampler). Bound the deviation of the sigmoid output."""
        from flowhip.nn.interp_weights_est import Simple
        torch.manual_seed(27)
        net = Simple(num_ch=[130, 64, 32], out_ch=2, filter_sz=[3, 3, 1]) \
            .to(_dev()).to(memory_format=torch.channels_last).eval()
        x = torch.randn(2, 130, 28, 64, device=_dev())
        with torch.no_grad():
            out_bf = net(x.to(torch.bfloat16)
                         .contiguous(memory_format=torch.channels_last))
            out_fp = net(x)
        err = (out_bf.float() - out_fp).abs().max().item()
        assert err < 0.03, err  # sigmoid-domain absolute deviation


class TestTrainingLearns:
    def test_loss_decreases_on_synthetic(self):
        """End-to-end on GPU: 25 optimizer steps on a fixed synthetic pair
        reduce the sequence loss substantially (all HIP kernels in the
        loop: corr GEMM/pyramid/lookup, conv_gemm, GRU gates, nconv,
        injection, loss)."""
        from flowhip.config.args import default_ncup_args
        from flowhip.models import build_model
        from flowhip import ops

        torch.manual_seed(1234)
        args = default_ncup_args(model="raft_nc_dbl", small=False,
                                 mixed_precision=True, dataset="sintel")
        model = build_model(args).to(_dev())
        model.train()
        opt = torch.optim.AdamW(model.parameters(), lr=2e-4)

        h, w = 128, 256
        g = torch.Generator().manual_seed(7)
        img1 = (torch.rand(2, 3, h, w, generator=g) * 255).to(_dev())
        img2 = (torch.rand(2, 3, h, w, generator=g) * 255).to(_dev())
        flow_gt = torch.nn.functional.interpolate(
            torch.randn(2, 2, 8, 16, generator=g) * 4, size=(h, w),
            mode="bilinear", align_corners=False).to(_dev())
        valid = torch.ones(2, h, w, device=_dev())

        losses = []
        for _ in range(25):
            opt.zero_grad(set_to_none=True)
            preds = model(img1, img2, iters=4)
            loss, _ = ops.sequence_loss(preds, flow_gt, valid, 0.85)
            loss.backward()
            torch.nn.utils.clip_grad_norm_(model.parameters(), 1.0)
            opt.step()
            losses.append(loss.item())
        assert all(torch.isfinite(torch.tensor(losses)))
        first = sum(losses[:5]) / 5
        last = sum(losses[-5:]) / 5
        assert last < 0.7 * first, (first, last)


class TestPacHIP:
    @pytest.mark.parametrize("K,dil,norm", [(3, 1, False), (5, 1, True),
                                            (5, 2, False)])
    def test_packernel_matches_torch(self, K, dil, norm):
        from flowhip.nn import pac
        torch.manual_seed(29)
        f = torch.randn(2, 6, 18, 24, device=_dev(), requires_grad=True)
        pad = (K - 1) * dil // 2
        k_hip, _ = pac.packernel2d(f, kernel_size=K, stride=1, padding=pad,
                                   dilation=dil, normalize_kernel=norm)
        f2 = f.detach().cpu().requires_grad_(True)
        k_ref, _ = pac.packernel2d(f2, kernel_size=K, stride=1, padding=pad,
                                   dilation=dil, normalize_kernel=norm)
        torch.testing.assert_close(k_hip.cpu(), k_ref, atol=1e-5, rtol=1e-5)
        g = torch.randn_like(k_ref)
        (k_hip * g.to(_dev())).sum().backward()
        (k_ref * g).sum().backward()
        torch.testing.assert_close(f.grad.cpu(), f2.grad, atol=1e-4,
                                   rtol=1e-4)

    @pytest.mark.parametrize("shared,pad", [(False, 2), (True, 2),
                                            (False, 0)])
    def test_pacconv_matches_torch(self, shared, pad):
        from flowhip.nn import pac
        torch.manual_seed(30)
        B, Ci, H, W, K = 2, 4, 16, 20, 5
        Co = Ci if shared else 3
        oh, ow = H + 2 * pad - (K - 1), W + 2 * pad - (K - 1)
        x = torch.randn(B, Ci, H, W, device=_dev(), requires_grad=True)
        kr = torch.rand(B, 1, K, K, oh, ow, device=_dev(),
                        requires_grad=True)
        w = (torch.randn(1, 1, K, K) if shared
             else torch.randn(Co, Ci, K, K)).to(_dev()).requires_grad_(True)
        b = torch.randn(Co, device=_dev(), requires_grad=True)

        out = pac.pacconv2d(x, kr, w, b, stride=1, padding=pad,
                            shared_filters=shared)
        x2 = x.detach().cpu().requires_grad_(True)
        kr2 = kr.detach().cpu().requires_grad_(True)
        w2 = w.detach().cpu().requires_grad_(True)
        b2 = b.detach().cpu().requires_grad_(True)
        ref = pac.pacconv2d(x2, kr2, w2, b2, stride=1, padding=pad,
                            shared_filters=shared)
        torch.testing.assert_close(out.cpu(), ref, atol=1e-4, rtol=1e-4)
        g = torch.randn_like(ref)
        (out * g.to(_dev())).sum().backward()
        (ref * g).sum().backward()
        torch.testing.assert_close(x.grad.cpu(), x2.grad, atol=1e-4, rtol=1e-4)
        torch.testing.assert_close(kr.grad.cpu(), kr2.grad, atol=1e-4, rtol=1e-4)
        torch.testing.assert_close(w.grad.cpu(), w2.grad, atol=1e-3, rtol=1e-3)
        torch.testing.assert_close(b.grad.cpu(), b2.grad, atol=1e-3, rtol=1e-3)

    def test_pac_upsampler_head_runs_on_gpu(self):
        from flowhip.nn.pac_upsampler import PacJointUpsample
        torch.manual_seed(31)
        # channels=1: the head folds multi-channel inputs to single-channel
        # batches (convert_to_single_channel, ref pac_upsampler.py:16)
        net = PacJointUpsample(factor=4, channels=1).to(_dev())
        lr = torch.randn(1, 2, 12, 16, device=_dev(), requires_grad=True)
        guide = torch.randn(1, 3, 48, 64, device=_dev())
        out = net(lr, guide)
        assert out.shape == (1, 2, 48, 64)
        out.sum().backward()
        assert lr.grad is not None and torch.isfinite(lr.grad).all()
