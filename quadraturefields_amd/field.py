"""Deformation / quadrature scalar field on the gfx950 kernels.

Mirrors ``Field`` of ``examples/field.py:130-270`` as the render path uses it
(``examples/utils.py:555-566``: ``field_net(x, return_grad=False)[0]``): hash grid (tcnn ``Encoding``)
followed by ``cat[x01, h] -> BasicDecoder``.  Inference is one fused launch; when autograd is recording the
differentiable route (HIP grid forward/backward + library GEMMs) is taken, which also serves ``field_grad`` --
including ``create_graph=True`` (the reference's default), through the second-order grid kernel.  The finetune
configuration (relu, hidden 32) infers through the deformation kernel; stage 2's (elu, hidden 16, train_field.py:238-252)
and the other two combinations through qf_field_grid_extract's point list (``field_utils`` uses its lattice source).
Stage 2's training step is ``field_loss``: the quadrature loss with a fused backward (qf_field_quadrature_loss).
"""
import numpy as np
import torch
from torch import nn

from . import _C
from . import tinycudann as tcnn


class BasicDecoder(nn.Module):
    """examples/field.py's BasicDecoder variant: like ngp.BasicDecoder plus ``bias_last``."""

    def __init__(self, input_dim, output_dim, activation, bias, layer=nn.Linear, num_layers=1, hidden_dim=128,
                 skip=[], bias_last=True):
        super().__init__()
        self.input_dim, self.output_dim, self.activation = input_dim, output_dim, activation
        self.num_layers, self.hidden_dim, self.skip = num_layers, hidden_dim, ([] if skip is None else skip)
        self.layers = nn.ModuleList(
            [layer(input_dim if i == 0 else hidden_dim, hidden_dim, bias=bias) for i in range(num_layers)])
        self.lout = layer(hidden_dim, output_dim, bias=bias_last)

    def forward(self, x):
        h = x
        for l in self.layers:
            h = self.activation(l(h))
        return self.lout(h)


class _DeformTrainFn(torch.autograd.Function):
    """Field.density with a fused backward (first order, parameter gradients only -- the input is data): forward = the
    inference kernel, backward = grid encode + qf_deform_mlp_backward + qf_grid_encode_backward."""

    @staticmethod
    def forward(ctx, x, table, w1, b1, w2, b2, wout, bout, module):
        x = _C.f32c(x.detach().reshape(-1, 3))
        enc = torch.empty((x.shape[0], 32), dtype=torch.float32, device=x.device)     # kept for the backward
        out = module._density_fused(x, None, enc_out=enc, compute_dtype="fp32")      # training is fp32 (class doc)
        ctx.save_for_backward(x, table, w1, b1, w2, b2, wout, bout, enc)
        ctx.module = module
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_out):
        x, table, w1, b1, w2, b2, wout, bout, enc = ctx.saved_tensors
        m = ctx.module
        n = x.shape[0]
        dev = x.device
        lib = _C.lib()
        table = _C.f32c(table.detach())
        ws = [_C.f32c(t.detach()) for t in (w1, b1, w2, b2, wout)]
        grads = [torch.zeros_like(t) for t in (w1, b1, w2, b2, wout, bout)]
        g_table = torch.zeros_like(table)
        if n:
            x01 = _C.f32c((x - m.xyz_min) / (m.xyz_max - m.xyz_min))
            desc = m.xyz_encoder.grid.desc
            d_enc = torch.empty((n, 32), dtype=torch.float32, device=dev)
            _C.check(lib.qf_deform_mlp_backward(_C.ptr(enc), _C.ptr(x01), _C.ptr(_C.f32c(d_out.reshape(-1))),
                                                *[_C.ptr(t) for t in ws], n, _C.ptr(d_enc), None,
                                                *[_C.ptr(t) for t in grads], _C.stream()), "qf_deform_mlp_backward")
            _C.grid_encode_backward(desc, table, x01, d_enc, n, g_table, None)
        return (None, g_table, *grads, None)


class _FieldLossFn(torch.autograd.Function):
    """Field.field_loss on qf_field_quadrature_loss: the forward launch gives the loss, the backward launch (with the
    upstream scalar read on the device) the five decoder gradients and d_enc, which qf_grid_encode_backward scatters
    into the table.  ``lout.bias`` is not an input: it does not enter the loss and keeps ``grad = None``."""

    @staticmethod
    def forward(ctx, table, w1, b1, w2, b2, wout, module, x, dirs, weights, weights_rev):
        x, dirs = _C.f32c(x.detach().reshape(-1, 3)), _C.f32c(dirs.detach().reshape(-1, 3))
        weights, weights_rev = _C.f32c(weights.detach().reshape(-1)), _C.f32c(weights_rev.detach().reshape(-1))
        ctx.save_for_backward(table, w1, b1, w2, b2, wout, x, dirs, weights, weights_rev)
        ctx.module = module
        return module._quadrature_loss(x, dirs, weights, weights_rev)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_loss):
        table, w1, b1, w2, b2, wout, x, dirs, weights, weights_rev = ctx.saved_tensors
        m = ctx.module
        n = x.shape[0]
        grads = [torch.zeros_like(t, dtype=torch.float32) for t in (w1, b1, w2, b2, wout)]
        g_table = torch.zeros_like(table, dtype=torch.float32)
        if n:
            table32 = _C.f32c(table.detach())
            d_enc = torch.empty((n, 32), dtype=torch.float32, device=x.device)
            m._quadrature_call(x, dirs, weights, weights_rev, upstream=_C.f32c(d_loss.detach().reshape(1)), d_enc=d_enc,
                               grads=grads)
            x01 = _C.f32c((x - m.xyz_min) / (m.xyz_max - m.xyz_min))
            _C.grid_encode_backward(m.xyz_encoder.grid.desc, table32, x01, d_enc, n, g_table, None)
        return (g_table, *grads, None, None, None, None, None)


class Field(nn.Module):
    def __init__(self, scale, back_prop=0, precision=16, log2_T=19, L=16, max_res=512, output_dim=1, min_res=16,
                 hidden_size=32, num_features=2, nl="elu", bias=True, bias_last=True):
        super().__init__()
        if nl not in self.ACTIVATIONS or output_dim != 1 or hidden_size not in (16, 32) or not bias or not bias_last:
            raise NotImplementedError("the fused kernels implement nl in {'relu', 'elu'}, hidden_size 16 or 32, "
                                      "output_dim 1 and both biases: the finetune configuration of "
                                      "train_finetune.py:387-399 (relu, hidden 32) and stage 2's of "
                                      "train_field.py:238-252 (elu, hidden 16)")
        self.output_dim = output_dim
        self.nl, self.hidden_size = nl, hidden_size
        # kept for API parity: ``precision`` selects nothing, ``compute_dtype`` (below) does
        self.dtype = torch.float16 if precision == 16 else torch.float32
        self.scale = scale
        self.register_buffer("center", torch.zeros(1, 3))
        self.register_buffer("xyz_min", -torch.ones(1, 3) * scale)
        self.register_buffer("xyz_max", torch.ones(1, 3) * scale)
        self.register_buffer("half_size", (self.xyz_max - self.xyz_min) / 2)
        self.back_prop = back_prop
        b = np.exp(np.log(max_res * scale / min_res) / (L - 1))
        self.xyz_encoder = tcnn.Encoding(
            n_input_dims=3,
            encoding_config={"otype": "Grid", "type": "Hash", "n_levels": L, "n_features_per_level": num_features,
                             "log2_hashmap_size": log2_T, "base_resolution": min_res, "per_level_scale": b,
                             "interpolation": "Linear"},
            dtype=self.dtype)
        self.decoder_field = BasicDecoder(input_dim=L * num_features + 3, output_dim=output_dim,
                                          activation=torch.nn.ELU() if nl == "elu" else torch.nn.ReLU(),
                                          bias=bias, num_layers=2,
                                          hidden_dim=hidden_size, skip=[], bias_last=bias_last)

    #: Activations of the decoder (field.py:172-175): torch.nn.ReLU() or torch.nn.ELU() (alpha 1).
    ACTIVATIONS = ("relu", "elu")

    @property
    def deform_kernel(self) -> bool:
        """True for the finetune configuration (relu, hidden 32), which the deformation kernel (qf_deform_field_forward)
        and its fused backward serve; every other accepted configuration infers through qf_field_grid_extract's point
        list and trains through the differentiable route (stage 2's loss has a fused step of its own: ``field_loss``)."""
        return self.nl == "relu" and self.hidden_size == 32

    #: Precision of the fused inference kernel: "fp32" (default; parity with the fp32 oracle to ~1e-6) or "fp16", the
    #: precision the reference builds this field in (``Field(precision=16)``, field.py:135-138,157-171: an fp16 tcnn
    #: ``Encoding`` whose fp16 output ``torch.cat`` promotes to fp32 for the fp32 ``BasicDecoder``): fp16 table, the 32
    #: encoding outputs rounded to fp16, x01 and the whole MLP fp32 (``qf_deform_field_forward_f16``).  ``precision=``
    #: does not select it -- a drop-in script that wants the reference's numbers sets ``Field.compute_dtype = "fp16"``
    #: once, before it builds its field.  Any other value raises ValueError at the first evaluation.  Only inference
    #: (autograd not recording) honours "fp16"; the training routes and ``field_grad`` are fp32 whatever it says.  The
    #: fp16 table is a copy of the fp32 master ``xyz_encoder.params``, kept while "fp16" is in use and rebuilt when the
    #: parameters change (an optimiser step -- torch's or ``optim.Adam`` -- or ``load_state_dict``): 0.41 GB more resident
    #: at the scripts' log2_T = 24.  Setting the instance's ``compute_dtype`` to anything else releases it at once; a
    #: class-level switch (``Field.compute_dtype = "fp32"``) releases it at the field's next evaluation.
    compute_dtype = "fp32"
    COMPUTE_DTYPES = ("fp32", "fp16")

    def __setattr__(self, name, value):
        if name == "compute_dtype" and value != "fp16":
            self.__dict__.pop("_half_cache", None)          # the fp16 table goes now, not at the next evaluation
        super().__setattr__(name, value)

    def _check_compute_dtype(self):
        if self.compute_dtype not in self.COMPUTE_DTYPES:
            raise ValueError(f"compute_dtype must be one of {', '.join(map(repr, self.COMPUTE_DTYPES))}, "
                             f"got {self.compute_dtype!r}")
        if self.compute_dtype == "fp32":
            self._half_cache = None

    def _half_table(self):
        """fp16 (round-to-nearest-even) copy of the fp32 table, keyed by the parameter's storage and version: built
        once per parameter change, never per call (203 M values at log2_T = 24)."""
        p = self.xyz_encoder.params
        key = (p.data_ptr(), p._version)
        cache = getattr(self, "_half_cache", None)
        if cache is None or cache.key != key:
            self._half_cache = cache = None    # the old copy goes before the new one is allocated
            half = p.detach().to(torch.float16).contiguous()
            cache = _C.StreamCached(key, half, [half])     # ordered for a consumer on another stream
            self._half_cache = cache
        return cache.get()

    def density(self, x, order=None, n_device=None):
        """[N,3] in [-scale, scale] -> [N,1].  field.py:186-203, one fused launch.  ``order`` (extension): int32
        processing permutation (``RayIntersector.coherent_layout`` / ``last_order``), cache locality only."""
        self._check_compute_dtype()
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            if self.fused_backward and self.deform_kernel and not x.requires_grad:
                d = self.decoder_field       # parameters train, the input is data: fused first-order backward
                return _DeformTrainFn.apply(x, self.xyz_encoder.params, d.layers[0].weight, d.layers[0].bias,
                                            d.layers[1].weight, d.layers[1].bias, d.lout.weight, d.lout.bias, self)
            x01 = (x.reshape(-1, 3) - self.xyz_min) / (self.xyz_max - self.xyz_min)
            h = self.xyz_encoder(x01 if self.back_prop else x01.detach())
            return self.decoder_field(torch.cat([x01, h], 1))
        return self._density_fused(x, order, n_device=n_device)

    #: Training route of ``density`` when only the parameters want gradients: True = fused HIP backward
    #: (``_DeformTrainFn``); the input-gradient / second-order route always goes through the hash-grid autograd Function.
    #: Also selects ``field_loss``'s route for stage 2's configuration (``_FieldLossFn``).
    fused_backward = True

    def _density_fused(self, x, order=None, enc_out=None, n_device=None, compute_dtype=None):
        """The inference kernel; ``compute_dtype`` None = the field's own."""
        x = _C.f32c(x.reshape(-1, 3))
        n = x.shape[0]
        out = torch.empty((n,), dtype=torch.float32, device=x.device)
        d = self.decoder_field
        w = [_C.f32c(t.detach()) for t in (d.layers[0].weight, d.layers[0].bias, d.layers[1].weight,
                                           d.layers[1].bias, d.lout.weight, d.lout.bias)]
        if not self.deform_kernel:
            return self._extract_points(x, w, n_device, compute_dtype)
        if (compute_dtype or self.compute_dtype) == "fp16":
            name, table = "qf_deform_field_forward_f16", self._half_table()
        else:
            name, table = "qf_deform_field_forward", self.xyz_encoder.params.detach()
        _C.check(getattr(_C.lib(), name)(
            self.xyz_encoder.grid.desc, _C.ptr(table), float(self.scale), 32,
            *[_C.ptr(t) for t in w], _C.ptr(x), n, _C.ptr(n_device, torch.int64),
            _C.ptr(order, torch.int32) if order is not None and order.shape[0] == n else None,
            _C.ptr(out), _C.ptr(enc_out), _C.stream()), name)
        return out[:, None]

    def _extract_points(self, x, w, n_device=None, compute_dtype=None):
        """Inference of a configuration other than the finetune one: qf_field_grid_extract on a point list, value only."""
        n = x.shape[0]
        out = torch.empty((n,), dtype=torch.float32, device=x.device)
        name, table = self.extract_entry(compute_dtype)
        _C.check(getattr(_C.lib(), name)(
            self.xyz_encoder.grid.desc, _C.ptr(table), float(self.scale), self.hidden_size, self.activation_code,
            *[_C.ptr(t) for t in w], None, 0, 0, 0, 1, _C.ptr(x), n, _C.ptr(n_device, torch.int64),
            _C.ptr(out), None, _C.stream()), name)
        return out[:, None]

    @property
    def activation_code(self) -> int:
        """QF_ACT_RELU / QF_ACT_ELU of include/qf_hip.h."""
        return 1 if self.nl == "elu" else 0

    def extract_entry(self, compute_dtype=None):
        """(qf_field_grid_extract entry point, table) for ``compute_dtype`` (None = the field's own)."""
        self._check_compute_dtype()
        if (compute_dtype or self.compute_dtype) == "fp16":
            return "qf_field_grid_extract_f16", self._half_table()
        return "qf_field_grid_extract", self.xyz_encoder.params.detach()

    def decoder_arrays(self):
        """w1, b1, w2, b2, wout, bout as contiguous fp32 tensors (the kernels' argument order)."""
        d = self.decoder_field
        return [_C.f32c(t.detach()) for t in (d.layers[0].weight, d.layers[0].bias, d.layers[1].weight,
                                              d.layers[1].bias, d.lout.weight, d.lout.bias)]

    def field(self, x, order=None, n_device=None):
        return self.density(x, order, n_device)[:, 0:self.output_dim]

    def forward(self, x, return_grad=True, order=None, n_device=None):
        """(field [N,1], field_grad [N,3] or None).  field.py:206-223.  ``order`` / ``n_device`` (extensions, inference
        only): see ``NGPRadianceField.forward``."""
        if not return_grad:
            return self.field(x, order, n_device), None
        if not x.requires_grad:
            x.requires_grad = True
        field = self.field(x)
        return field, self.field_grad(x, field, create_graph=True)

    def field_grad(self, coords, field, create_graph=True):
        """d field / d coords, field.py:229-238 (``create_graph=True`` keeps it differentiable for the losses of
        field.py:240-270)."""
        field = field.flatten()
        return torch.autograd.grad(field, [coords], grad_outputs=torch.ones_like(field), create_graph=create_graph,
                                   retain_graph=True)[0]

    def compute_field_loss(self, weights, weights_rev, field_norm, view_dirs):
        """field.py:253-259."""
        view_dirs = view_dirs / torch.norm(view_dirs, dim=1, keepdim=True)
        return torch.abs(torch.maximum(weights.detach(), weights_rev.detach())
                         - torch.abs(torch.sum(field_norm * view_dirs.detach(), 1))).mean()

    @property
    def quadrature_kernel(self) -> bool:
        """True for stage 2's configuration (elu, hidden 16, ``back_prop`` false), which qf_field_quadrature_loss
        serves: ``field_loss`` with a fused backward and ``value_and_grad``."""
        return self.nl == "elu" and self.hidden_size == 16 and not self.back_prop

    def _quadrature_call(self, x, dirs=None, weights=None, weights_rev=None, upstream=None, loss=None, value=None,
                         grad=None, d_enc=None, grads=None, workspace=None):
        """qf_field_quadrature_loss on contiguous fp32 tensors (None -> NULL); the training routes are fp32."""
        p = _C.ptr
        _C.check(_C.lib().qf_field_quadrature_loss(
            self.xyz_encoder.grid.desc, p(_C.f32c(self.xyz_encoder.params.detach())), float(self.scale),
            self.hidden_size, self.activation_code, *[p(t) for t in self.decoder_arrays()], p(x), p(dirs), p(weights),
            p(weights_rev), x.shape[0], p(upstream), p(loss, torch.float64), p(value), p(grad), p(d_enc),
            *([p(t) for t in grads] if grads is not None else [None] * 5), p(workspace, torch.uint8),
            0 if workspace is None else workspace.numel(), _C.stream()), "qf_field_quadrature_loss")

    def _quadrature_loss(self, x, dirs, weights, weights_rev):
        """The loss alone, as a 0-d fp32 tensor (summed in fp64 on the device, rounded once)."""
        loss = torch.empty((1,), dtype=torch.float64, device=x.device)
        ws = torch.empty((_C.FIELD_LOSS_WORKSPACE_BYTES,), dtype=torch.uint8, device=x.device)
        self._quadrature_call(x, dirs, weights, weights_rev, loss=loss, workspace=ws)
        return loss[0].to(torch.float32)

    def field_loss(self, positions, weights, weights_rev, view_dirs):
        """``compute_field_loss(weights, weights_rev, self(positions)[1], view_dirs)`` (train_field.py:346-350) as one
        call (extension).  For stage 2's configuration with ``fused_backward`` it is one fused launch forward and one
        backward (qf_field_quadrature_loss) plus the table scatter; otherwise exactly that expression on the
        differentiable route.  ``positions`` is data: it gets no gradient on the fused route."""
        if not (self.quadrature_kernel and self.fused_backward):
            return self.compute_field_loss(weights, weights_rev, self(positions)[1], view_dirs)
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            d = self.decoder_field
            return _FieldLossFn.apply(self.xyz_encoder.params, d.layers[0].weight, d.layers[0].bias, d.layers[1].weight,
                                      d.layers[1].bias, d.lout.weight, self, positions, view_dirs, weights, weights_rev)
        return self._quadrature_loss(_C.f32c(positions.detach().reshape(-1, 3)), _C.f32c(view_dirs.detach().reshape(-1, 3)),
                                     _C.f32c(weights.detach().reshape(-1)), _C.f32c(weights_rev.detach().reshape(-1)))

    def value_and_grad(self, x):
        """(field [N,1], d field / dx [N,3]) for inspection and plotting (extension, inference only: nothing is
        recorded).  Stage 2's configuration: one launch of qf_field_quadrature_loss with these two outputs; any other:
        ``forward(return_grad=True)``, detached."""
        if not self.quadrature_kernel:
            with torch.enable_grad():
                value, grad = self(x.detach().clone())
            return value.detach(), grad.detach()
        x = _C.f32c(x.detach().reshape(-1, 3))
        value = torch.empty((x.shape[0],), dtype=torch.float32, device=x.device)
        grad = torch.empty((x.shape[0], 3), dtype=torch.float32, device=x.device)
        self._quadrature_call(x, value=value, grad=grad)
        return value[:, None], grad

    def compute_abs_loss(self, field_norm):
        """field.py:261-264."""
        return torch.linalg.norm(field_norm, ord=1, dim=1).mean()
