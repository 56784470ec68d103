"""torch.autograd glue for the training step.  Every forward AND backward below is a HIP kernel
behind the C ABI; torch only records the graph, slices/concatenates buffers and owns .grad accumulation.

Used by SkipConnMLP / the model classes whenever gradients are enabled and something requires them; inference
keeps using the fused MFMA kernels.
"""
import torch
from torch.autograd import Function

from . import config, ops


_NAN = {}


def _nan_scalar(device):
    t = _NAN.get(device)
    if t is None:
        t = _NAN[device] = torch.full((1, 1), float("nan"), device=device, dtype=torch.float32)
    return t


def needs_grad(*tensors) -> bool:
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


class LinearFn(Function):
    """y = W . act([x0 | x1]) + b  (src/neural_blocks.py:288-296).  config.train_precision selects the three GEMMs:
    "bf16x3": split-bf16 MFMA kernels of csrc/train_gemm.hip (activation derivative fused into the input gradient);
    "fp32": exact f32-MFMA Linear, act_backward and weight-gradient kernels."""

    @staticmethod
    def forward(ctx, x0, x1, W, b, act, packs=None):
        """packs: None or (packed W, packed W^T | None) from ops.train_pack_many (SkipConnMLP._forward_train packs every Linear of
        the network with one launch per step) -- only meaningful in the "bf16x3" training arithmetic."""
        ctx.act = act
        ctx.fast = config.train_precision == "bf16x3"
        ctx.save_for_backward(x0, x1 if x1 is not None else torch.empty(0, device=x0.device), W)
        ctx.has_x1 = x1 is not None
        ctx.has_b = b is not None
        ctx.packed_t = packs[1] if (packs is not None and ctx.fast) else None
        return ops.linear_f32(x0, W, b, pre_act=act, x1=x1, split_bf16=ctx.fast,
                              packed=packs[0] if (packs is not None and ctx.fast) else None)

    @staticmethod
    def backward(ctx, gy):
        x0, x1, W = ctx.saved_tensors
        x1 = x1 if ctx.has_x1 else None
        gy = gy.contiguous()
        in0 = x0.shape[1]
        gx0 = gx1 = gW = gb = None
        want0, want1 = ctx.needs_input_grad[0], ctx.has_x1 and ctx.needs_input_grad[1]
        want_w = ctx.needs_input_grad[2] or (ctx.has_b and ctx.needs_input_grad[3])
        N, out = x0.shape[0], gy.shape[1]
        if (ctx.fast and want0 and want_w and ctx.packed_t is not None and (x1 is None or (in0 == 256 and x1.shape[1] <= 256))
                and ops.linear_bwd_fused_ok(N, out, in0)):
            # round 5: input gradient + weight gradient of a source in ONE pass over dY and that source (csrc/train_bwd.hip): the
            # 256 wide hidden input, an init Linear's narrow input, and the narrow second source of a skip layer as a call of its own
            in1 = x1.shape[1] if x1 is not None else 0
            gx0, gW, gb = ops.linear_bwd_fused(gy, x0, ctx.act, ctx.packed_t, in1=in1, want_bias=ctx.has_b)
            if x1 is not None:
                if want1 and ops.linear_bwd_fused_ok(N, out, in1):
                    gx1, _, _ = ops.linear_bwd_fused(gy, x1, ctx.act, ctx.packed_t, dW=gW, col0=in0)
                else:
                    ops.linear_wgrad_cols(x1, gy, ctx.act, gW, in0)
                    if want1:
                        _, gx1 = ops.linear_dgrad(gy, W, x0, ctx.act, x1, False, True, packed_t=ctx.packed_t)
            return gx0, gx1, gW, gb, None, None
        if (want0 or want1) and ctx.fast:
            gx0, gx1 = ops.linear_dgrad(gy, W, x0, ctx.act, x1, want0, want1, packed_t=ctx.packed_t)
        elif want0 or want1:
            g_act = ops.linear_f32(gy, W.t().contiguous(), None)  # [N, in0+in1] = dL/d act(x)
            if want0:
                g0 = g_act[:, :in0].contiguous()
                gx0 = ops.act_backward(x0, g0, ctx.act) if ctx.act != "none" else g0
            if want1:
                g1 = g_act[:, in0:].contiguous()
                gx1 = ops.act_backward(x1, g1, ctx.act) if ctx.act != "none" else g1
        if ctx.needs_input_grad[2] or (ctx.has_b and ctx.needs_input_grad[3]):
            gW, gb = ops.linear_wgrad(x0, gy, ctx.act, x1, want_bias=ctx.has_b, split_bf16=ctx.fast)
        return gx0, gx1, gW, gb, None, None


class HashEncodeFn(Function):
    """HashEncoder.forward (src/neural_blocks.py:139-193): gradients w.r.t. the tables (scatter) and, for
    deformation models whose canonical positions are predicted, w.r.t. the positions."""

    @staticmethod
    def forward(ctx, x, tables, include_input):
        ctx.save_for_backward(x, tables)
        ctx.include_input = include_input
        return ops.hash_encode(x, tables, include_input)

    @staticmethod
    def backward(ctx, g):
        x, tables = ctx.saved_tensors
        g = g.contiguous()
        gx = gt = None
        if ctx.needs_input_grad[0]:
            gx = ops.hash_encode_backward_input(x, tables, g, ctx.include_input)
        if ctx.needs_input_grad[1]:
            gt = ops.hash_encode_backward(x, g, ctx.include_input)
        return gx, gt, None


class HashInitFn(Function):
    """The init rows cat([p, enc(p)]) = [x | x | features] of a hash-encoded SkipConnMLP without a latent (src/neural_blocks.py:139-193,
    283-287) as ONE node and ONE kernel (round 6: hash_encode + cat forward; slice copy + scatter backward before).  The backward reads
    the rows' gradient in place: tables through the scatter kernel, positions (D-NeRF's warped points) through the input-gradient
    kernel, which adds both copies of x like autograd's accumulation did."""

    @staticmethod
    def forward(ctx, x, tables, include_input):
        ctx.save_for_backward(x, tables)
        ctx.include_input = include_input
        return ops.hash_encode_rows(x, tables, include_input, 1)

    @staticmethod
    def backward(ctx, g):
        x, tables = ctx.saved_tensors
        g = g.contiguous()
        gx = gt = None
        if ctx.needs_input_grad[0]:
            gx = ops.hash_encode_backward_input_rows(x, tables, g, ctx.include_input, 1)
        if ctx.needs_input_grad[1]:
            gt = ops.hash_encode_backward_rows(x, g, 3 * (1 + int(ctx.include_input)))
        return gx, gt, None


class FourierEncodeFn(Function):
    """FourierEncoder.forward (src/neural_blocks.py:52, src/utils.py:14-17) with the gradient w.r.t. the positions (a deformation field
    in front of a Fourier-encoded canonical model).  The basis is a frozen parameter: no gradient."""

    @staticmethod
    def forward(ctx, x, basis, scale):
        ctx.save_for_backward(x, basis)
        ctx.scale = scale
        return ops.fourier_encode(x, basis, scale)

    @staticmethod
    def backward(ctx, g):
        x, basis = ctx.saved_tensors
        gx = ops.fourier_encode_backward_input(x, basis, ctx.scale, g.contiguous()) if ctx.needs_input_grad[0] else None
        return gx, None, None


class FourierInitFn(Function):
    """The init rows cat([p, enc(p), latent]) = [x | sin | cos | latent] of a Fourier-encoded SkipConnMLP (src/neural_blocks.py:283-287)
    as ONE node and ONE kernel each way (the counterpart of HashInitFn): the backward reads the rows' gradient in place -- positions
    through the input-gradient kernel, which adds the raw columns' gradient; the latent's gradient is the view of its columns."""

    @staticmethod
    def forward(ctx, x, basis, scale, latent):
        ctx.save_for_backward(x, basis)
        ctx.scale = scale
        return ops.fourier_rows(x, basis, scale, latent)

    @staticmethod
    def backward(ctx, g):
        x, basis = ctx.saved_tensors
        g = g.contiguous()
        D, F = basis.shape
        gx = ops.fourier_encode_backward_input(x, basis, ctx.scale, g, col0=D, lead=True) if ctx.needs_input_grad[0] else None
        gl = g[:, D + 2 * F:] if ctx.needs_input_grad[3] else None
        return gx, None, None, gl


class PlainHeadFn(Function):
    """PlainNeRF between its two networks in training (src/nerf.py:338-357, src/refl.py:190-207): first_out [N, 1 + C] ->
    (density [N], the View MLP's init rows [N, 5 + C]) by one kernel; the backward writes [g_density | g_rows[:, 5:]] side by side
    (and the points' three columns when they carry a gradient: D-NeRF)."""

    @staticmethod
    def forward(ctx, first_out, pts, dirs, pre=None):
        if pre is not None:
            # (round 6: the one-launch training forward wrote density and rows itself; `first_out` is a placeholder nobody reads)
            return pre
        return ops.plain_head_rows(first_out, pts, dirs)

    @staticmethod
    def backward(ctx, g_density, g_rows):
        g_first, g_pts = ops.plain_head_rows_backward(g_density, g_rows.contiguous(), ctx.needs_input_grad[1])
        return g_first, g_pts, None, None


class HashJvpFn(Function):
    """d hash_encode(x)/dx . tangent (rows [tangent | per-level features]: na_hash_encode_jvp) as a graph node: the gradient
    w.r.t. the tables is the adjoint scatter na_hash_encode_jvp_backward (the features are linear in the tables); positions
    and tangent carry no gradient (floor() has none, and the callers' directions are constants)."""

    @staticmethod
    def forward(ctx, x, tables, tangent, include_input):
        ctx.save_for_backward(x, tangent)
        ctx.include_input = include_input
        return ops.hash_encode_jvp(x, tables, tangent, include_input)

    @staticmethod
    def backward(ctx, g):
        x, tangent = ctx.saved_tensors
        gt = ops.hash_encode_jvp_backward(x, tangent, g.contiguous(), ctx.include_input) if ctx.needs_input_grad[1] else None
        return None, gt, None, None


class LaplaceDensityFn(Function):
    """VolSDF density 1/beta * laplace_cdf(-sdf, beta) (src/nerf.py:985-990, src/utils.py:50-58)."""

    @staticmethod
    def forward(ctx, sdf, beta):
        ctx.save_for_backward(sdf, beta)
        return ops.laplace_density(sdf, beta)

    @staticmethod
    def backward(ctx, g):
        sdf, beta = ctx.saved_tensors
        g_sdf, g_beta = ops.laplace_density_backward(sdf, beta, g.contiguous(), want_beta=ctx.needs_input_grad[1])
        return g_sdf, (g_beta.reshape(beta.shape) if g_beta is not None else None)


class BezierWarpFn(Function):
    """DynamicNeRF spline warp (src/nerf.py:1267-1278) -> (warped pts, dp, rigidity [, refl_latent when n_rl > 0]); gradient
    w.r.t. the estimator output and the (pass-through) points."""

    @staticmethod
    def forward(ctx, est, pts, t, n_ctrl, n_rl=0):
        ctx.save_for_backward(est, t)
        ctx.n_ctrl, ctx.n_rl = n_ctrl, n_rl
        return ops.bezier_warp(est, pts, t, n_ctrl, n_rl)

    @staticmethod
    def backward(ctx, g_pts, g_dp, g_rig, g_enc=None):
        est, t = ctx.saved_tensors
        g_est = ops.bezier_warp_backward(est, t, ctx.n_ctrl, g_pts, g_dp, g_rig, ctx.n_rl, g_enc)
        return g_est, (g_pts if ctx.needs_input_grad[1] else None), None, None, None


class SigmoidFn(Function):
    @staticmethod
    def forward(ctx, x, kind):
        ctx.kind = kind
        ctx.save_for_backward(x)
        return ops.sigmoid(x, kind)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return ops.sigmoid_backward(x, g.contiguous(), ctx.kind), None


class PosLinearCombineFn(Function):
    """(sigmoid(lin)/2 + 0.5) * pos[..., :C] (src/refl.py:288-290)."""

    @staticmethod
    def forward(ctx, lin, pos, c_out):
        ctx.c_out = c_out
        ctx.save_for_backward(lin, pos)
        with torch.no_grad():
            return ops.pos_linear_combine(lin, pos, c_out)

    @staticmethod
    def backward(ctx, g):
        lin, pos = ctx.saved_tensors
        g_lin, g_pos = ops.pos_linear_combine_backward(lin, pos, g.contiguous(), ctx.c_out, ctx.needs_input_grad[0],
                                                       ctx.needs_input_grad[1])
        return g_lin, g_pos, None


class ShShadeFn(Function):
    """act(eval_sh(order, coeffs.reshape(..., 3, K), normalize(dirs))) (src/refl.py:726-731, src/spherical_harmonics.py:55-106) as one
    node: coeffs [..., 3 K], dirs [R, 3] (row n -> ray n % R).  The directions carry no gradient."""

    @staticmethod
    def forward(ctx, coeffs, dirs, order, kind):
        ctx.order, ctx.kind, ctx.shape = order, kind, coeffs.shape
        rgb, pre = ops.sh_shade(coeffs, dirs, order, kind, want_pre=True)
        ctx.save_for_backward(pre, dirs)
        return rgb

    @staticmethod
    def backward(ctx, g):
        if ctx.needs_input_grad[1]:
            raise NotImplementedError("ShShadeFn: d(colour)/d(view direction) has no HIP backward")
        pre, dirs = ctx.saved_tensors
        g_c = ops.sh_shade_backward(g.contiguous().reshape(-1, 3), pre.reshape(-1, 3), dirs, ctx.order, ctx.kind)
        return g_c.reshape(ctx.shape), None, None, None


class ActDerivFn(Function):
    """m = act'(x) as a differentiable node (its own derivative is act''(x): -sin for sin, 0 for LeakyReLU)."""

    @staticmethod
    def forward(ctx, x, act):
        ctx.act = act
        ctx.save_for_backward(x)
        return ops.act_deriv(x, act, 1)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        if ctx.act != "sin":
            return torch.zeros_like(x), None
        return ops.mul_bcast(ops.act_deriv(x, ctx.act, 2), g.contiguous().unsqueeze(0)).squeeze(0), None


class MulBcastFn(Function):
    """out[j] = a * b[j]: the multiplier row a [N,K] is shared by the J tangent rows b [J,N,K]."""

    @staticmethod
    def forward(ctx, a, b):
        ctx.save_for_backward(a, b)
        return ops.mul_bcast(a, b)

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        g = g.contiguous()
        ga = ops.mul_reduce(g, b) if ctx.needs_input_grad[0] else None
        gb = ops.mul_bcast(a, g) if ctx.needs_input_grad[1] else None
        return ga, gb


class EikonalFn(Function):
    """utils.eikonal_loss (src/utils.py:31) on tangent-major normals [3, N]."""

    @staticmethod
    def forward(ctx, normals):
        ctx.save_for_backward(normals)
        return ops.eikonal_loss(normals)

    @staticmethod
    def backward(ctx, g):
        (normals,) = ctx.saved_tensors
        return ops.eikonal_loss_backward(normals, g.contiguous())


class RowNormalizeFn(Function):
    """F.normalize(x, dim=-1) over rows of width <= 64 (NeRFAE --normalize-latent, src/nerf.py:824)."""

    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return ops.row_normalize(x)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return ops.row_normalize_backward(x, g.contiguous())


class RowSqnormMeanFn(Function):
    """torch.linalg.norm(x, dim=-1).square().mean() (NeRFAE's latent_l2_loss, src/nerf.py:811)."""

    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return ops.row_sqnorm_mean(x)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return ops.row_sqnorm_mean_backward(x, g.contiguous())


class CompositeFn(Function):
    """alpha_from_density + volumetric_integrate + sky (src/nerf.py:60-80,96-98).  Returns (out, alpha, weights);
    alpha/weights are auxiliary (non-differentiable) outputs."""

    @staticmethod
    def forward(ctx, density, feat, ts, rays, softplus, bg, rand=None):
        out, alpha, weights = ops.composite(density, feat, ts, rays, softplus=softplus, bg=bg, rand=rand)
        ctx.save_for_backward(density, feat, ts, rays)
        ctx.softplus, ctx.bg, ctx.rand = softplus, bg, rand  # (rand: the per-ray draw of bg "random", a constant)
        ctx.mark_non_differentiable(alpha, weights)
        ctx.set_materialize_grads(False)  # (no zero-filled [T, R] gradients for the two auxiliary outputs: two fill launches per step)
        return out, alpha, weights

    @staticmethod
    def backward(ctx, g_out, _ga, _gw):
        density, feat, ts, rays = ctx.saved_tensors
        gd, gf = ops.composite_backward(density, feat, ts, rays, g_out.contiguous(), ctx.softplus, ctx.bg, rand=ctx.rand)
        return gd, gf, None, None, None, None, None


class CompositeRayTsFn(Function):
    """CompositeFn over per-ray steps ts_ray [..., T] (the fine pass of coarse -> fine training; csrc/composite_rayts.hip).  Returns
    (out, alpha, weights); alpha / weights are auxiliary outputs, ts_ray and rays constants: no gradient flows through the sample
    positions."""

    @staticmethod
    def forward(ctx, density, feat, ts_ray, rays, softplus, bg, rand=None):
        out, alpha, weights = ops.composite_rayts(density, feat, ts_ray, rays, softplus=softplus, bg=bg, rand=rand)
        ctx.save_for_backward(density, feat, ts_ray, rays)
        ctx.softplus, ctx.bg, ctx.rand = softplus, bg, rand
        ctx.mark_non_differentiable(alpha, weights)
        ctx.set_materialize_grads(False)
        return out, alpha, weights

    @staticmethod
    def backward(ctx, g_out, _ga, _gw):
        density, feat, ts_ray, rays = ctx.saved_tensors
        gd, gf = ops.composite_rayts_backward(density, feat, ts_ray, rays, g_out.contiguous(), ctx.softplus, ctx.bg, rand=ctx.rand)
        return gd, gf, None, None, None, None, None


class SplitHeadFn(Function):
    """(y[..., 0] contiguous, y[..., 1:] as a view) of a network output [.., 1 + C] -- PlainNeRF's density | intermediate
    (src/nerf.py:338-342).  The same values as the two slices; the point is the BACKWARD: autograd's own slice gradients are a
    zero-filled [.., 1 + C] tensor per slice plus their sum (fill + copy + fill + copy + add over a [N, 65] tensor: ~110 us per
    training step at N = 262 144); here the two gradients are written side by side into one uninitialised buffer: two copies."""

    @staticmethod
    def forward(ctx, y):
        ctx.shape = y.shape
        tail = y[..., 1:]
        return y[..., 0].contiguous(), tail

    @staticmethod
    def backward(ctx, g_head, g_tail):
        g = torch.empty(ctx.shape, device=(g_head if g_head is not None else g_tail).device, dtype=torch.float32)
        if g_head is not None:
            g[..., 0].copy_(g_head)
        else:
            g[..., 0].zero_()
        if g_tail is not None:
            g[..., 1:].copy_(g_tail)
        else:
            g[..., 1:].zero_()
        return g


class MlpTrainFn(Function):
    """A whole SkipConnMLP (src/neural_blocks.py:279-296) as ONE autograd node (round 5): the forward is the same chain of training
    Linears as LinearFn; the backward walks the layers itself -- the one-pass input + weight gradient kernel per source
    (csrc/train_bwd.hip) WITHOUT its reduction -- and sums the partial gradients of ALL Linears with one launch at the end
    (14 reduce launches and their gaps per PlainNeRF step before), with one host round trip through autograd instead of one per
    Linear.  Used when every Linear of the network takes the fused kernels (SkipConnMLP._mlp_fn_ok); otherwise the per-layer nodes."""

    @staticmethod
    def forward(ctx, init, spec, *params):
        """spec: {"act": str, "skips": [bool per hidden layer], "packs": [(packed W, packed W^T)] per Linear};
        params: W, b of init, the hidden layers, out (b may be None)."""
        act, skips, packs = spec["act"], spec["skips"], spec["packs"]
        Ws, bs = params[0::2], params[1::2]
        L = len(Ws)
        acts = ["none"] + [act] * (L - 1)
        x1s = [None] + [init if s else None for s in skips] + [None]
        pre = spec.get("pre")
        if pre is not None:
            # round 6: the forward has run already -- both networks of PlainNeRF in ONE launch of the layer-synchronous engine
            # (ops.train_plain_view_ls), which left every Linear's output rows in HBM: pre = ([L - 1 row tensors], the network's output)
            rows, x = pre
            assert len(rows) == L - 1 and all(r.shape == (init.shape[0], W.shape[0]) for r, W in zip(rows, Ws)), (L, [r.shape for r in rows])
            xs = [init] + list(rows)
            if x is None:
                # the network's output went straight into its consumer's format (PlainNeRF's `first`: density + the View MLP's init
                # rows, PlainHeadFn with `pre`): a placeholder of the right shape keeps the graph's edges, its values are never read
                # -- and if a future caller does read them it gets NaN, not stale memory (one cached scalar per device, broadcast: no launch)
                x = _nan_scalar(init.device).expand(init.shape[0], Ws[-1].shape[0])
        else:
            xs, x = [], init
            for li in range(L):
                xs.append(x)
                x = ops.linear_f32(x, Ws[li], bs[li], pre_act=acts[li], x1=x1s[li], split_bf16=True, packed=packs[li][0])
        ctx.save_for_backward(*xs, *Ws)
        ctx.L, ctx.acts, ctx.has_x1 = L, acts, [t is not None for t in x1s]
        ctx.has_b = [b is not None for b in bs]
        ctx.packed_t = [p[1] for p in packs]
        return x

    @staticmethod
    def backward(ctx, gy):
        L = ctx.L
        saved = ctx.saved_tensors
        xs, Ws = saved[:L], saved[L:]
        init = xs[0]
        g = gy.contiguous()
        pending, gWs, gbs, g_init = [], [None] * L, [None] * L, None
        for li in range(L - 1, -1, -1):
            x0, W = xs[li], Ws[li]
            out, in0 = W.shape[0], x0.shape[1]
            in1 = init.shape[1] if ctx.has_x1[li] else 0
            nW = out * (in0 + in1)
            pad = (-nW) % 4
            buf = torch.empty(nW + pad + (out if ctx.has_b[li] else 0), device=g.device, dtype=torch.float32)
            dW = buf[:nW].view(out, in0 + in1)
            db = buf[nW + pad:] if ctx.has_b[li] else None
            # (the init Linear's input gradient takes the skip layers' gradient of the same tensor as an addend: no add launch)
            fuse_add = li == 0 and g_init is not None and in0 <= 128
            gx0, ws, npart = ops.linear_bwd_partials(g, x0, ctx.acts[li], ctx.packed_t[li], 0, ctx.has_b[li], add=g_init if fuse_add else None)
            if fuse_add:
                g_init = None
            pending.append((ws, npart, out, in0, dW, 0, db))
            if in1:
                gx1, ws1, np1 = ops.linear_bwd_partials(g, init, ctx.acts[li], ctx.packed_t[li], in0, False)
                pending.append((ws1, np1, out, in1, dW, in0, None))
                g_init = gx1 if g_init is None else g_init + gx1
            gWs[li], gbs[li] = dW, db
            if li == 0:
                g_init = gx0 if g_init is None else g_init + gx0
            else:
                g = gx0
        ops.train_reduce_many(pending)
        grads = []
        for li in range(L):
            grads += [gWs[li], gbs[li]]
        return (g_init if ctx.needs_input_grad[0] else None, None, *grads)


class ViewInputFn(Function):
    """cat([x, dir_to_elev_azim(view)]) with the view direction of a ray broadcast along its samples (src/refl.py:190-207) as one
    kernel; the directions carry no gradient (they come from the camera), the points get their three columns back."""

    @staticmethod
    def forward(ctx, x, dirs):
        return ops.view_rows(x, dirs)

    @staticmethod
    def backward(ctx, g):
        return (g[..., :3] if ctx.needs_input_grad[0] else None), None


class GridTVFn(Function):
    """nerf.total_variation (src/nerf.py:381-399) of a grid [s0,s1,s2,C] at flat indices (ops.grid_tv: one launch); backward is
    ops.grid_tv_backward, one launch that recomputes the differences and reads the upstream scalar on the device."""

    @staticmethod
    def forward(ctx, grid, idxs, trusted):
        ctx.trusted = trusted
        ctx.save_for_backward(grid, idxs)
        return ops.grid_tv(grid, idxs, trusted)

    @staticmethod
    def backward(ctx, g):
        grid, idxs = ctx.saved_tensors
        return ops.grid_tv_backward(grid, idxs, g.contiguous(), True), None, None  # (the forward checked the indices)


def _voxel_lookup_save(ctx, pts_arg, densities, rgb, grid_radius, rays, pts, ts, order=None):
    """What the lookup node of every voxel head keeps (pts_arg: index of `pts` among forward's arguments): only the positions -- the
    rays (None where the RGB head reads explicit pts) and explicit pts or ts; the cells are recomputed -- and the grids only when explicit
    pts require a gradient (DynamicNeRFVoxel's warped points), for the gather that returns it."""
    ctx.grid_radius, ctx.S, ctx.order = grid_radius, densities.shape[0], order
    ctx.explicit = pts is not None
    ctx.pts_grad = ctx.explicit and ctx.needs_input_grad[pts_arg]
    ctx.save_for_backward(rays, pts if ctx.explicit else ts, *((densities, rgb) if ctx.pts_grad else ()))


def _voxel_lookup_backward(ctx, g, scatter, gather, fill=None):
    """(g_densities, g_rgb, g_pts) of a lookup node.  g: the gradients of its outputs, (g_raw,) or (g_raw, g_sh); fill: per output the
    trailing shape of the zeros that stand in for a gradient autograd did not materialise (a node that asks for that); scatter(*g, rays=, pts= | ts=) is the head's scatter-add into the two grids, run if either wants a gradient; gather(*g, pts,
    rays, densities, rgb) is its position gradient, run for explicit pts that require one (the rays x ts form has none)."""
    rays, pos, *grids = ctx.saved_tensors
    if fill is not None:
        batch = tuple(pos.shape[:-1]) if ctx.explicit else (pos.shape[0],) + tuple(rays.shape[:-1])
        g = [x if x is not None else pos.new_zeros(batch + tail) for x, tail in zip(g, fill)]
    g = [x.contiguous() for x in g]
    kw = {"rays": rays, "pts": pos} if ctx.explicit else {"rays": rays, "ts": pos}
    g_den = g_rgb = g_pts = None
    if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
        g_den, g_rgb = scatter(*g, **kw)
    if ctx.pts_grad:
        g_pts = gather(*g, pos, rays, *grids)
    return g_den, g_rgb, g_pts


class VoxelSampleFn(Function):
    """raw [..., 1 + C] of NeRFVoxel's grid lookup (ops.voxel_sample); backward scatters into the two grids (ops.voxel_sample_backward)
    and gives explicit pts their gradient (ops.voxel_sample_backward_pts): `_voxel_lookup_save` / `_voxel_lookup_backward`."""

    @staticmethod
    def forward(ctx, densities, rgb, grid_radius, pts, rays, ts):
        _voxel_lookup_save(ctx, 3, densities, rgb, grid_radius, rays, pts, ts)
        return ops.voxel_sample(densities, rgb, grid_radius, pts=pts, rays=rays, ts=ts)

    @staticmethod
    def backward(ctx, g):
        g_den, g_rgb, g_pts = _voxel_lookup_backward(
            ctx, (g,), lambda g, **kw: ops.voxel_sample_backward(g, ctx.S, ctx.grid_radius, **kw),
            lambda g, pts, rays, den, rgb: ops.voxel_sample_backward_pts(g, pts, den, rgb, ctx.grid_radius))
        return g_den, g_rgb, None, g_pts, None, None


class VoxelMaskRowsFn(Function):
    """The training route of a sparsified NeRFVoxel: the lookup's rows [..., C] with the dead samples' rows replaced by
    (fill0, 0, ..., 0) (ops.voxel_mask_rows; flags uint8 [...], ops.voxel_live_samples).  fill0 is ops.VOXEL_DEAD_DENSITY on the raw rows
    -- a density whose softplus is exactly 0 -- and 0 on the pos-linear-view head's sh column.  The backward is the same kernel on the
    gradient with fill0 = 0: the scatter behind it receives exact zeros for dead samples.  With all flags set both directions return
    their input's bits."""

    @staticmethod
    def forward(ctx, x, flags, fill0=ops.VOXEL_DEAD_DENSITY):
        ctx.save_for_backward(flags)
        return ops.voxel_mask_rows(x, flags, fill0)

    @staticmethod
    def backward(ctx, g):
        (flags,) = ctx.saved_tensors
        return ops.voxel_mask_rows(g.contiguous(), flags, 0.0), None, None


class VoxelPlvSampleFn(Function):
    """(raw [..., 4], sh [...]) of NeRFVoxel's lookup with the pos-linear-view head (ops.voxel_plv_sample); the rays' directions are the
    head's view.  Backward: ops.voxel_plv_sample_backward / ops.voxel_plv_sample_backward_pts, as VoxelSampleFn."""

    @staticmethod
    def forward(ctx, densities, rgb, grid_radius, rays, pts, ts):
        _voxel_lookup_save(ctx, 4, densities, rgb, grid_radius, rays, pts, ts, ops.PLV_CHANNELS.get(rgb.shape[-1]))
        ctx.set_materialize_grads(False)
        return ops.voxel_plv_sample(densities, rgb, grid_radius, rays, pts=pts, ts=ts)

    @staticmethod
    def backward(ctx, g_raw, g_sh):
        g_den, g_rgb, g_pts = _voxel_lookup_backward(
            ctx, (g_raw, g_sh), lambda g, s, **kw: ops.voxel_plv_sample_backward(g, s, ctx.S, ctx.order, ctx.grid_radius, **kw),
            lambda g, s, pts, rays, den, rgb: ops.voxel_plv_sample_backward_pts(g, s, pts, rays, den, rgb, ctx.grid_radius), fill=((4,), ()))
        return g_den, g_rgb, None, None, g_pts, None


class VoxelShSampleFn(Function):
    """raw [..., 4] = [density | s_r s_g s_b] of NeRFVoxel's lookup with the spherical-harmonic colour head (ops.voxel_sh_sample).
    Backward: ops.voxel_sh_sample_backward / ops.voxel_sh_sample_backward_pts, as VoxelSampleFn."""

    @staticmethod
    def forward(ctx, densities, rgb, order, grid_radius, rays, pts, ts):
        _voxel_lookup_save(ctx, 5, densities, rgb, grid_radius, rays, pts, ts, order)
        return ops.voxel_sh_sample(densities, rgb, order, grid_radius, rays, pts=pts, ts=ts)

    @staticmethod
    def backward(ctx, g_raw):
        g_den, g_rgb, g_pts = _voxel_lookup_backward(
            ctx, (g_raw,), lambda g, **kw: ops.voxel_sh_sample_backward(g, ctx.S, ctx.order, ctx.grid_radius, **kw),
            lambda g, pts, rays, den, rgb: ops.voxel_sh_sample_backward_pts(g, pts, rays, den, rgb, ctx.order, ctx.grid_radius))
        return g_den, g_rgb, None, None, None, g_pts, None


class DynVoxelWarpFn(Function):
    """(warped, dp, rigidity) of DynamicNeRFVoxel's deformation (ops.dyn_voxel_warp, one launch); all three are differentiable --
    `warped` feeds the canonical lookup, `dp` and `rigidity` the offset regularisers -- and backward is one scatter-add into the two
    grids (ops.dyn_voxel_warp_backward).  pts and t carry no gradient (the positions are a leaf in the reference)."""

    @staticmethod
    def forward(ctx, ctrl_pts_grid, rigidity_grid, pts, t, spline, grid_radius):
        warped, dp, rigidity = ops.dyn_voxel_warp(pts, t, ctrl_pts_grid, rigidity_grid, spline, grid_radius)
        ctx.save_for_backward(pts, t, dp, rigidity)
        ctx.S, ctx.spline, ctx.grid_radius = rigidity_grid.shape[0], spline, grid_radius
        ctx.set_materialize_grads(False)
        return warped, dp, rigidity

    @staticmethod
    def backward(ctx, g_warped, g_dp, g_rigidity):
        pts, t, dp, rigidity = ctx.saved_tensors
        g_ctrl, g_rig = ops.dyn_voxel_warp_backward(pts, t, dp, rigidity, ctx.S, ctx.spline, ctx.grid_radius, g_warped, g_dp, g_rigidity)
        return g_ctrl, g_rig, None, None, None, None


class GridSplineLenFn(Function):
    """mean arc length of the splines stored in the rows idxs of a control-point grid (ops.grid_spline_len: one launch); backward is
    ops.grid_spline_len_backward, one launch that recomputes the points and reads the upstream scalar on the device."""

    @staticmethod
    def forward(ctx, grid, idxs, trusted):
        ctx.save_for_backward(grid, idxs)
        return ops.grid_spline_len(grid, idxs, trusted)

    @staticmethod
    def backward(ctx, g):
        grid, idxs = ctx.saved_tensors
        return ops.grid_spline_len_backward(grid, idxs, g.contiguous(), True), None, None  # (the forward checked the indices)


class DynVoxelSplineLenFn(Function):
    """mean over the samples of w * arc length of the sample's interpolated spline (ops.dyn_voxel_spline_len: one launch); backward is
    one scatter-add into ctrl_pts_grid (ops.dyn_voxel_spline_len_backward).  pts and w carry no gradient (the reference detaches the
    weights, and the positions are a leaf)."""

    @staticmethod
    def forward(ctx, ctrl_pts_grid, pts, w, spline, grid_radius):
        ctx.save_for_backward(ctrl_pts_grid, pts, *(() if w is None else (w,)))
        ctx.spline, ctx.grid_radius = spline, grid_radius
        return ops.dyn_voxel_spline_len(pts, ctrl_pts_grid, spline, grid_radius, w)

    @staticmethod
    def backward(ctx, g):
        ctrl, pts, *w = ctx.saved_tensors
        g_ctrl = ops.dyn_voxel_spline_len_backward(pts, ctrl, ctx.spline, ctx.grid_radius, g.contiguous(), w[0] if w else None)
        return g_ctrl, None, None, None, None


class DynVoxelJacQuadFn(Function):
    """v . (J_dp v) per sample (ops.dyn_voxel_jac_quad without a rigidity grid: one launch), J_dp the Jacobian of DynamicNeRFVoxel's dp
    w.r.t. the unwarped position; differentiable w.r.t. ctrl_pts_grid, in which it is linear: backward is one scatter-add
    (ops.dyn_voxel_jac_quad_backward) that needs neither the grid nor the forward's output.  pts, t and v carry no gradient.  The
    dp * rigidity form has no graph in the reference (src/utils.py:471-477) and is evaluated by the operator directly."""

    @staticmethod
    def forward(ctx, ctrl_pts_grid, pts, t, v, spline, grid_radius):
        ctx.save_for_backward(pts, t, *(() if v is None else (v,)))
        ctx.S, ctx.spline, ctx.grid_radius = ctrl_pts_grid.shape[0], spline, grid_radius
        return ops.dyn_voxel_jac_quad(pts, t, ctrl_pts_grid, None, spline, grid_radius, v)

    @staticmethod
    def backward(ctx, g):
        pts, t, *v = ctx.saved_tensors
        g_ctrl = ops.dyn_voxel_jac_quad_backward(pts, t, ctx.S, ctx.spline, ctx.grid_radius, g.contiguous(), v[0] if v else None)
        return g_ctrl, None, None, None, None, None


class SSIMFn(Function):
    """ssim [N,C] of the channel-last pair x, y [N,H,W,C] (ops.ssim); backward is ops.ssim_backward, one launch that recomputes the
    moments per tile.  The gradient goes to x only: y is the reference image."""

    @staticmethod
    def forward(ctx, x, y, flag):
        ctx.flag = flag
        ctx.save_for_backward(x, y)
        return ops.ssim(x, y, 1.0, flag)[0].contiguous()

    @staticmethod
    def backward(ctx, g):
        x, y = ctx.saved_tensors
        return ops.ssim_backward(x, y, g.contiguous(), 1.0, ctx.flag), None, None


class ImageLossFn(Function):
    """the reference's loss wrapper of got against ref [..., 3] (ops.image_loss: one launch); backward is ops.image_loss_backward, one
    elementwise launch that reads the upstream scalar on the device.  The gradient goes to got only: ref is the label."""

    @staticmethod
    def forward(ctx, got, ref, loss_fns, color_spaces, tone_map, gamma):
        ctx.cfg = (tuple(loss_fns), tuple(color_spaces), bool(tone_map), float(gamma))
        loss, stats = ops.image_loss(got, ref, *ctx.cfg)
        ctx.save_for_backward(got, ref, stats)
        return loss

    @staticmethod
    def backward(ctx, g):
        got, ref, stats = ctx.saved_tensors
        return ops.image_loss_backward(got, ref, stats, g.contiguous(), *ctx.cfg), None, None, None, None, None
