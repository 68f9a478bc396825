"""Host-side model of the Switch-NeRF train hot path on top of libswn_hip.so.

Mirrors, for the building.yaml wiring (NeRFMoE, external gate + LayerNorm, top-1 expertmlp, batched capacity path):
  * models/nerf_moe.py:103-455  NeRFMoE            -> SwitchNeRF (parameters, state_dict layout, forward)
  * rendering.py:15-494         render_rays        -> SwitchNeRF.render / rendering.render_rays
  * runner.py:1077-1123, 646-686 training step      -> SwitchNeRF.train_step (loss, backward, Adam)
(paths relative to /root/reference/switch_nerf/).  All arithmetic on points runs in HIP kernels through the C ABI;
torch only owns the device buffers, the stream, and a handful of per-ray (N_rays x 75) tensors.

MI355X-first design notes
  * the whole ray batch (e.g. 8192 x 256 = 2M points, ~30 GB of bf16 activations) is processed in ONE pass: the
    reference's model chunks (rendering.py:354) survive only as routing *segments* (capacity / ranking / l_aux are
    per segment), so every kernel is launched once per step over all segments - 288 GB of HBM makes chunking for
    memory unnecessary;
  * dispatch and the backward scatter never materialise: the expert chain gathers its input rows through the
    routing permutation, and the front backward gathers the expert input-gradient rows through tok2row;
  * the direction / appearance part of layer "2" is constant along a ray: it is folded into a per-ray bias
    (N_rays x 128) instead of being concatenated to every point (331 -> 256 input features on the hot GEMM);
  * master weights are fp32 in [in, out] layout in one flat buffer (one Adam launch, one gradient all-reduce);
    compute copies (bf16 or fp32) in [out, in] (forward) and [in, out] (backward-data) are refreshed after Adam.
"""
from __future__ import annotations

import contextlib
import os
import math
from collections import namedtuple
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib, hier, ops, optim
from .noise import DeviceNoise

BUILDING = dict(model_dim=256, num_experts=8, expert_layers=7, skips=(3,), pos_xyz_dim=12, pos_dir_dim=4,
                appearance_dim=48, appearance_count=10, gate_hidden=256, gate_layers=2, layer2_out=128)


def _ceil_to(x, m):
    return (x + m - 1) // m * m


# What a forward's heads launch instead of the model's own (fused, plain, affine) ones: _net_forward's `head`, kept in the context.
ShHead = namedtuple("ShHead", "dirs want_coef")             # the spherical-harmonics contraction against dirs [groups, 3]; also c["coef"]
CoefHead = namedtuple("CoefHead", "out inner_sigmoid")      # a Mega-NeRF cell's coefficient rows, written into out [n, 3 B + 1]

_EXP_RECORD_STREAM = os.environ.get("SWN_EXP_RECORD_STREAM") == "1"      # see SwitchNeRF._join_side_outputs (read once, experiment only)


def resolve_kernel_switches(env=None) -> dict:
    """The kernel-selection switches of a model, resolved ONCE (SwitchNeRF.__init__ reads the process environment through this; no
    forward / backward looks at os.environ).  Defaults = the shipped kernel set; the SWN_* variables are experiment / test knobs:
      front_geom (SWN_FRONT_GEOM, 7)      dense front chains: 7 / 6 = the persistent 256-row geometry, 1 = the 64-row kernels
      chain_geom (SWN_CHAIN_GEOM, 7)      expert chains: include/swn.h swn_chain_desc.geometry (1, 2, 4, 5, 6, 7)
      tail_geom (SWN_TAIL_GEOM, 1)        the separate tail backward chain: 6 / 7 = persistent geometry (measured slower: off)
      fused_tail (SWN_FUSED_TAIL, on)     dense tail + heads inside the expert forward launch (chain_big.hip tag 7)
      fused_tail_bwd (SWN_FUSED_TAIL_BWD, on)   tail backward + combine backward in front of the expert backward chain (tag 8)
      fused_dwsig (SWN_FUSED_DWSIG, on)   the sigma head's weight gradient from tag 8's combine pass
      fused_heads (SWN_NO_FUSED_HEADS unset)    sigma / colour heads inside the tail forward chain (swn.h: heads_raw)
      overlap (SWN_NO_OVERLAP != 1)       side-stream overlap of the expert weight gradients and the per-ray launches"""
    e = os.environ if env is None else env
    return dict(front_geom=int(e.get("SWN_FRONT_GEOM", "7")), chain_geom=int(e.get("SWN_CHAIN_GEOM", "7")),
                tail_geom=int(e.get("SWN_TAIL_GEOM", "1")), fused_tail=e.get("SWN_FUSED_TAIL", "1") != "0",
                fused_tail_bwd=e.get("SWN_FUSED_TAIL_BWD", "1") != "0", fused_dwsig=e.get("SWN_FUSED_DWSIG", "1") != "0",
                fused_heads=e.get("SWN_NO_FUSED_HEADS") is None, overlap=e.get("SWN_NO_OVERLAP", "0") != "1")


def c_esz(dtype) -> int:
    return 4 if dtype == torch.float32 else 2

class LossScaler:
    """torch.cuda.amp.GradScaler's contract (the reference trains fp16 with it: runner.py:483 `GradScaler(enabled=hparams.amp)`,
    :679 `scaler.scale(loss).backward()`, scaler.step / update): the loss gradient is multiplied by `scale`, the optimizer step
    is skipped when a gradient is not finite (scale *= backoff_factor), and after growth_interval clean steps scale *= growth_factor.
    Same defaults as torch."""

    def __init__(self, init_scale=65536.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000):
        self.scale, self.growth_factor, self.backoff_factor, self.growth_interval = float(init_scale), growth_factor, backoff_factor, growth_interval
        self._good = 0
        self.skipped = 0

    def update(self, found_inf: bool):
        if found_inf:
            self.scale *= self.backoff_factor
            self._good = 0
            self.skipped += 1
        else:
            self._good += 1
            if self._good >= self.growth_interval:
                self.scale *= self.growth_factor
                self._good = 0

    def state_dict(self):
        return {"scale": self.scale, "growth_factor": self.growth_factor, "backoff_factor": self.backoff_factor,
                "growth_interval": self.growth_interval, "_growth_tracker": self._good}

    def load_state_dict(self, sd):
        """GradScaler.load_state_dict's keys (the reference saves scaler.state_dict() under 'scaler', runner.py:2806)."""
        if not sd:
            return
        self.scale = float(sd.get("scale", self.scale))
        self.growth_factor = float(sd.get("growth_factor", self.growth_factor))
        self.backoff_factor = float(sd.get("backoff_factor", self.backoff_factor))
        self.growth_interval = int(sd.get("growth_interval", self.growth_interval))
        self._good = int(sd.get("_growth_tracker", 0))


DYNCAP_EP_ERROR = ("capacity_factor = 0 (dynamic capacity, nothing dropped) is not supported with expert parallelism: the exchange "
                   "buffers are sized by a static capacity; use capacity_factor > 0, or < 0 (the dynamic capacity clamped at the static one)")
ACCUM_OWNER_TAIL_ERROR = ("gradient accumulation (set_accumulation) is not built for expert parallelism with owner_tail=True: the tail's "
                          "gradient is summed on the experts' ranks inside the step")


CHECK_FINITE_OWNER_TAIL_ERROR = ("the finite guard (check_finite) is not built for expert parallelism with owner_tail=True: the tail's "
                                 "optimizer state is stepped on the experts' ranks inside the step")


def accumulation_rule(iteration: int, steps: int) -> bool:
    """The reference's should_accumulate (runner.py:589): iteration `iteration` (0-based) of a run with `steps` accumulation steps
    only accumulates; the optimizer steps on every steps-th iteration."""
    return (int(iteration) + 1) % int(steps) != 0


class SwitchNeRF:
    def __init__(self, cfg: dict = BUILDING, dtype=torch.bfloat16, device="cuda", capacity_factor=1.0,
                 batch_prioritized=True, moe_l_aux_wt=5e-4, lr=5e-4, seed=0, gate_noise=-1.0, kernel_switches=None):
        self.cfg, self.dtype, self.dev = dict(cfg), dtype, torch.device(device)
        # the kernel selection is resolved HERE, once (environment knobs included); set_kernel_switches() changes it afterwards
        self.sw = resolve_kernel_switches()
        self._env_overrides = {k: v for k, v in sorted(os.environ.items()) if k.startswith("SWN_")}
        if kernel_switches:
            self.set_kernel_switches(**kernel_switches)
        # the 16-bit compute type selects the build of the library: bfloat16 (amp_use_bfloat16) or IEEE half (the reference's default
        # autocast dtype; BASELINE configs[4] "fp16 MFMA") - see _lib.use_half.  fp16 trains with loss scaling like the reference.
        if dtype == torch.float16:
            _lib.use_half("f16")
        elif dtype == torch.bfloat16:
            _lib.use_half("bf16")
        self.loss_scaler = LossScaler() if dtype == torch.float16 else None
        # capacity_factor (--moe_capacity_factor, opts.py:118): > 0 a static capacity; 0 the reference's dynamic capacity, nothing dropped
        # (the packed no-drop row space below); < 0 the dynamic capacity clamped at the static one of |cf| - see capacity()
        self.cf, self.bpr, self.wt, self.lr = capacity_factor, batch_prioritized, moe_l_aux_wt, lr
        # --gate_noise (opts.py:208, default -1 = off): a TRAINING forward adds gate_noise * randn / E to the router's logits
        # (tutel_moe_layer_nobatch.py:119-122).  gate_noise_draw: a [P, E] tensor to use as that draw (tests), else drawn per forward.
        self.gate_noise, self.gate_noise_draw = float(gate_noise), None
        self.base_lr = lr             # undecayed rate ('initial_lr' of the reference's ExponentialLR); self.lr = the current rate
        spec = self._configure(cfg)
        if self.affine or self.sh_deg is not None:      # the colour transform / the spherical-harmonics contraction runs in the heads' own
            self.sw.update(fused_heads=False, fused_tail=False, fused_tail_bwd=False)      # launches (swn_heads_affine_*, swn_heads_sh_*), behind the unfused tail
        self.spec, off = {}, 0
        self.n_dense = None           # elements of the flat buffer before the first expert parameter (all of it for dense models)
        for i, (name, shape) in enumerate(spec):
            if i == getattr(self, "_n_dense_spec", len(spec)):
                self.n_dense = off
            n = int(np.prod(shape))
            self.spec[name] = (off, shape)
            off += _ceil_to(n, 64)
        self.n_flat = off
        if self.n_dense is None:
            self.n_dense = off
        z = lambda: torch.zeros(self.n_flat, dtype=torch.float32, device=self.dev)
        self.flat, self.grad, self.m, self.v = z(), z(), z(), z()
        self.p = {k: self.flat[o:o + int(np.prod(s))].view(s) for k, (o, s) in self.spec.items()}
        self.g = {k: self.grad[o:o + int(np.prod(s))].view(s) for k, (o, s) in self.spec.items()}
        self.step_count = 0
        # compute copies
        self.wf: Dict[str, torch.Tensor] = {}
        self.wb: Dict[str, torch.Tensor] = {}
        self._init_random(seed)
        self._bufs = {}
        self.profile = False          # bench.py: record HIP events around the major launches
        self.events: Dict[str, list] = {}
        # side HIP stream: the HBM-bound expert weight-gradient GEMMs overlap with the rest of the backward pass
        self.side = torch.cuda.Stream(device=self.dev) if self.dev.type == "cuda" else None
        self.overlap = self.sw["overlap"]      # side-stream overlap of the expert weight gradients
        self._kernel_sel = {}         # kernel_set(): what the last forward / backward selected
        self.ep = None                # parallel.ExpertParallel: experts sharded over ranks, tokens exchanged (set_expert_parallel)
        self.expert_wgrad_splits = 0         # row splits of the legacy expert weight-gradient launch (0 = heuristic)
        self.noise = DeviceNoise()    # the seeded device noise's state (set_device_noise); a BackgroundScene lends its own while it is on

    def _configure(self, cfg):
        """Sets the network dimensions and returns the flat parameter layout [(name, shape)]; Linear weights are [in, out]."""
        assert tuple(cfg["skips"]) == (3,) or len(cfg["skips"]) <= 1, "one skip connection supported"
        if cfg.get("sh_deg") is not None:
            raise NotImplementedError("sh_deg: spherical-harmonics colour is the dense NeRF's (DenseNeRF); NeRFMoE asserts a 4-channel sigma "
                                      "layer when pos_dir_dim == 0 (models/nerf_moe.py:186-189) and cannot carry the coefficients")
        M, E, L, G, H2 = cfg["model_dim"], cfg["num_experts"], cfg["expert_layers"], cfg["gate_hidden"], cfg["layer2_out"]
        assert G == M, "external gate width must equal model_dim (building.yaml)"
        self.hash = cfg.get("hash")                  # multiresolution hash-grid input encoding (ops.hash_encode_fwd) or None
        self.in_xyz = 3 + 6 * cfg["pos_xyz_dim"] if self.hash is None else 2 * self.hash["n_levels"]
        self.in_dir = 3 + 6 * cfg["pos_dir_dim"]
        self.KP = _ceil_to(self.in_xyz, 64)          # padded PE width (chain K granularity)
        self.DP = _ceil_to(self.in_dir, 8)
        # --affine_appearance (opts.py:55; models/nerf_moe.py:153-161): the appearance embedding feeds a Linear(appearance_dim, 12) whose
        # output transforms the colour head's output per image (:436-438) and no longer enters layer "2" (:161, :426)
        self.affine = bool(cfg.get("affine_appearance", False))
        if self.affine and cfg["appearance_dim"] <= 0:
            raise ValueError("affine_appearance needs appearance_dim > 0 (models/nerf_moe.py:154)")
        self.n_ray_feat = self.in_dir + (0 if self.affine else cfg["appearance_dim"])
        spec = [("xyz.w", (self.KP, M)), ("xyz.b", (M,)), ("gate0.w", (M, G)), ("gate0.b", (G,)),
                ("gate1.w", (G, G)), ("gate1.b", (G,)), ("ln.w", (G,)), ("ln.b", (G,)), ("wg", (E, G))]
        spec += [("l1.w", (M, M)), ("l1.b", (M,)), ("l2h.w", (M, H2)), ("l2r.w", (self.n_ray_feat, H2)), ("l2.b", (H2,)),
                 ("sigma.w", (M,)), ("sigma.b", (1,)), ("color.w", (3, H2)), ("color.b", (3,)),
                 ("emb", (cfg["appearance_count"], cfg["appearance_dim"]))]
        # the expert parameters come LAST in the flat buffer: under expert parallelism only the dense prefix is all-reduced
        # (the reference keeps the experts out of DDP, models/nerf_moe.py:139, 1037-1039); hash table: see below
        self._expert_spec = []
        for l in range(L):
            self._expert_spec += [(f"exp{l}.w", (E, M, M)), (f"exp{l}.b", (E, M))]
        self.L, self.M, self.E, self.G, self.H2 = L, M, E, G, H2
        self._chain_weights = ["xyz", "gate0", "gate1", "l1", "l2h"] + [f"exp{l}" for l in range(L)]
        self._fwd_only_weights = {"xyz"}              # first layer: no input gradient, no transposed copy
        if self.hash is not None:                     # trainable encoding: the first layer's input gradient feeds the table
            spec.append(("hash.table", (self.hash["n_levels"], 1 << self.hash["log2_table"], 2)))
            self._fwd_only_weights = set()
        if self.affine:                               # appended to the dense prefix: no other parameter moves
            spec += [("affine.w", (12, cfg["appearance_dim"])), ("affine.b", (12,))]
        self._n_dense_spec = len(spec)
        return spec + self._expert_spec

    @contextlib.contextmanager
    def _timed(self, name):
        if not self.profile:
            yield
            return
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        yield
        b.record()
        self.events.setdefault(name, []).append((a, b))

    # ------------------------------------------------------------------------------------------ parameters
    def _init_random(self, seed):
        """torch.nn.Linear-style init (U(-1/sqrt(in), 1/sqrt(in))) drawn in the reference's state_dict layout."""
        import sys, os
        g = torch.Generator().manual_seed(seed)
        cfg = self.cfg

        def lin(out_f, in_f):
            b = 1.0 / math.sqrt(in_f)
            return ((torch.rand(out_f, in_f, generator=g) * 2 - 1) * b), ((torch.rand(out_f, generator=g) * 2 - 1) * b)
        sd = {}
        M, E, L, G, H2 = self.M, self.E, self.L, self.G, self.H2
        sd["layers.xyz.fcs.0.weight"], sd["layers.xyz.fcs.0.bias"] = lin(M, self.in_xyz)
        for l in range(L):
            w = torch.empty(E, M, M)
            b = torch.empty(E, 1, M)
            for e in range(E):
                wt, bt = lin(M, M)
                w[e], b[e, 0] = wt.t(), bt
            sd[f"layers.0.experts.0.weights.{l}"], sd[f"layers.0.experts.0.bias.{l}"] = w, b
        sd["layers.0.gates.0.wg.weight"] = lin(E, G)[0]
        sd["layers.1.fcs.0.weight"], sd["layers.1.fcs.0.bias"] = lin(M, M)
        sd["layers.2.fcs.0.weight"], sd["layers.2.fcs.0.bias"] = lin(H2, M + self.n_ray_feat)
        sd["layers.sigma.fcs.0.weight"], sd["layers.sigma.fcs.0.bias"] = lin(1, M)
        sd["layers.color.fcs.0.weight"], sd["layers.color.fcs.0.bias"] = lin(3, H2)
        sd["layers.moe_external_gate.fcs.0.weight"], sd["layers.moe_external_gate.fcs.0.bias"] = lin(G, M)
        sd["layers.moe_external_gate.fcs.1.weight"], sd["layers.moe_external_gate.fcs.1.bias"] = lin(G, G)
        sd["layers.gate_input_norm.weight"], sd["layers.gate_input_norm.bias"] = torch.ones(G), torch.zeros(G)
        sd["embedding_a.weight"] = torch.randn(cfg["appearance_count"], cfg["appearance_dim"], generator=g)
        if self.hash is not None:         # instant-NGP initialisation: U(-1e-4, 1e-4)
            sd["embedding_xyz.table"] = (torch.rand(self.spec["hash.table"][1], generator=g) * 2 - 1) * 1e-4
        if self.affine:
            sd["affine.weight"], sd["affine.bias"] = lin(12, cfg["appearance_dim"])
        self.load_state_dict(sd)

    def load_state_dict(self, sd):
        """Accepts the reference's NeRFMoE.state_dict() key layout - as saved (`module.` prefix of
        the DDP wrapper, expertmlp stacking) or after the reference's convert_to_seqexperts (per-expert modules,
        models/model_utils.py:12-28); values torch or numpy.  See checkpoint.py."""
        from . import checkpoint
        self._load_ref_layout(checkpoint.to_expertmlp(sd), self.p)
        self.refresh_compute_copies()

    def _views(self, flat):
        """name -> view dict over a flat buffer laid out like the parameters (gradients, Adam moments)."""
        return {k: flat[o:o + int(np.prod(s))].view(s) for k, (o, s) in self.spec.items()}

    def _load_ref_layout(self, sd, p):
        """Inverse of _to_ref_layout: tensors keyed like the reference's state_dict -> the flat-buffer views `p`."""
        def t(k):
            v = sd[k]
            v = torch.from_numpy(np.asarray(v)) if not torch.is_tensor(v) else v
            return v.detach().to(torch.float32).to(self.dev)
        M = self.M
        with torch.no_grad():
            p["xyz.w"].zero_()
            p["xyz.w"][: self.in_xyz] = t("layers.xyz.fcs.0.weight").t()
            p["xyz.b"].copy_(t("layers.xyz.fcs.0.bias"))
            p["gate0.w"].copy_(t("layers.moe_external_gate.fcs.0.weight").t())
            p["gate0.b"].copy_(t("layers.moe_external_gate.fcs.0.bias"))
            p["gate1.w"].copy_(t("layers.moe_external_gate.fcs.1.weight").t())
            p["gate1.b"].copy_(t("layers.moe_external_gate.fcs.1.bias"))
            p["ln.w"].copy_(t("layers.gate_input_norm.weight"))
            p["ln.b"].copy_(t("layers.gate_input_norm.bias"))
            p["wg"].copy_(t("layers.0.gates.0.wg.weight"))
            for l in range(self.L):
                p[f"exp{l}.w"].copy_(t(f"layers.0.experts.0.weights.{l}"))
                p[f"exp{l}.b"].copy_(t(f"layers.0.experts.0.bias.{l}").view(self.E, M))
            p["l1.w"].copy_(t("layers.1.fcs.0.weight").t())
            p["l1.b"].copy_(t("layers.1.fcs.0.bias"))
            w2 = t("layers.2.fcs.0.weight")
            p["l2h.w"].copy_(w2[:, :M].t())
            p["l2r.w"].copy_(w2[:, M:].t())
            p["l2.b"].copy_(t("layers.2.fcs.0.bias"))
            p["sigma.w"].copy_(t("layers.sigma.fcs.0.weight").view(-1))
            p["sigma.b"].copy_(t("layers.sigma.fcs.0.bias"))
            p["color.w"].copy_(t("layers.color.fcs.0.weight"))
            p["color.b"].copy_(t("layers.color.fcs.0.bias"))
            p["emb"].copy_(t("embedding_a.weight"))
            if self.hash is not None:
                p["hash.table"].copy_(t("embedding_xyz.table"))
            if self.affine:
                p["affine.w"].copy_(t("affine.weight"))
                p["affine.b"].copy_(t("affine.bias"))

    def _to_ref_layout(self, d):
        M = self.M
        out = {}
        out["layers.xyz.fcs.0.weight"] = d["xyz.w"][: self.in_xyz].t().contiguous()
        out["layers.xyz.fcs.0.bias"] = d["xyz.b"].clone()
        out["layers.moe_external_gate.fcs.0.weight"] = d["gate0.w"].t().contiguous()
        out["layers.moe_external_gate.fcs.0.bias"] = d["gate0.b"].clone()
        out["layers.moe_external_gate.fcs.1.weight"] = d["gate1.w"].t().contiguous()
        out["layers.moe_external_gate.fcs.1.bias"] = d["gate1.b"].clone()
        out["layers.gate_input_norm.weight"] = d["ln.w"].clone()
        out["layers.gate_input_norm.bias"] = d["ln.b"].clone()
        out["layers.0.gates.0.wg.weight"] = d["wg"].clone()
        for l in range(self.L):
            out[f"layers.0.experts.0.weights.{l}"] = d[f"exp{l}.w"].clone()
            out[f"layers.0.experts.0.bias.{l}"] = d[f"exp{l}.b"].view(self.E, 1, M).clone()
        out["layers.1.fcs.0.weight"] = d["l1.w"].t().contiguous()
        out["layers.1.fcs.0.bias"] = d["l1.b"].clone()
        out["layers.2.fcs.0.weight"] = torch.cat([d["l2h.w"].t(), d["l2r.w"].t()], 1).contiguous()
        out["layers.2.fcs.0.bias"] = d["l2.b"].clone()
        out["layers.sigma.fcs.0.weight"] = d["sigma.w"].view(1, -1).clone()
        out["layers.sigma.fcs.0.bias"] = d["sigma.b"].clone()
        out["layers.color.fcs.0.weight"] = d["color.w"].clone()
        out["layers.color.fcs.0.bias"] = d["color.b"].clone()
        out["embedding_a.weight"] = d["emb"].clone()
        if self.hash is not None:
            out["embedding_xyz.table"] = d["hash.table"].clone()
        if self.affine:      # (an affine model lists its keys in the order the reference registers them: checkpoint.param_order)
            from . import checkpoint
            out["affine.weight"], out["affine.bias"] = d["affine.w"].clone(), d["affine.b"].clone()
            out = {k: out[k] for k in checkpoint.param_order(out.keys())}
        return out

    def state_dict(self, layout="expertmlp", prefix=""):
        """Parameters in the reference's key layout (so checkpoints are interchangeable): layout "expertmlp" (what the
        reference trains and saves) or "seqexperts" (what its evaluation loads after convert_to_seqexperts)."""
        sd = self._to_ref_layout(self.p)
        if layout == "seqexperts":
            from . import checkpoint
            return checkpoint.to_seqexperts(sd, prefix)
        assert layout == "expertmlp"
        return {prefix + k: v for k, v in sd.items()}

    def grad_dict(self):
        """Gradients in the reference's key layout (for parity tests)."""
        return self._to_ref_layout(self.g)

    def refresh_compute_copies(self):
        """fp32 master [in, out] -> MFMA-fragment-major compute copies: forward (N=out, K=in), backward (N=in, K=out)."""
        if self.dev.type != "cuda":      # a host-resident model holds parameters only (key layout, checkpoints): no kernel can run on it
            return
        pairs = []
        for n in self._chain_weights:
            w = self.p[n + ".w"]
            w3 = w if w.dim() == 3 else w.unsqueeze(0)
            if n not in self.wf:
                self.wf[n] = ops.pack_weights(w3, self.dtype, True)
                if n not in self._fwd_only_weights:
                    self.wb[n] = ops.pack_weights(w3, self.dtype, False)
            else:
                pairs.append((w3, self.wf[n], True))
                if n in self.wb:
                    pairs.append((w3, self.wb[n], False))
        # the front chains on the persistent 256-row geometry (chain_big.hip, geometry 7) run every layer with K = 256: the first layer's
        # 128-row weight (75 -> 256, PE padded to 128) is packed zero-padded to 256 rows
        if self._front_big():
            w3 = self.p["xyz.w"].unsqueeze(0)
            if "xyz_pad" not in self.wf:
                self.wf["xyz_pad"] = ops.pack_weights_padded(w3, self.dtype, True, 256)
            else:
                pairs.append((w3, self.wf["xyz_pad"], True, 256))
        # the tail BACKWARD layers likewise: dh2 (128 features) under the backward-data copy of layer "2" padded in K; the tail folded into
        # the expert forward chain: layer "2" (256 -> 128) zero-padded to 256 outputs
        for fwd, d, want in ((False, self.wb, self._tail_big() or self._tail_fused()), (True, self.wf, self._tail_fused())):
            if "l2h_pad" in d:
                pairs.append((self.p["l2h.w"].unsqueeze(0), d["l2h_pad"], fwd, 0, 256))
            elif want:
                self._l2h_pad(fwd)
        if pairs:
            ops.repack_weights_batched(pairs)      # one launch (was 23 of ~5 us each: a tenth of the step at 1024 rays per GPU)
        if self._flat_param is not None:           # the copies now match the master weights as of this version of flat_param
            self._packed_version = self._flat_param._version

    def kernel_set(self) -> dict:
        """The kernel selection the LAST forward / backward of this model resolved to (what the SWN_* environment switches and the
        shapes added up to): expert chain geometry (7 = persistent phase-shifted 256-row tiles, accumulators start at the bias), front
        chain geometry, the dense tail inside the expert forward launch (tag 7), its backward + combine backward in front of the expert
        backward chain (tag 8), the sigma head's weight gradient from that launch's combine pass, side-stream overlap of the expert
        weight gradients, expert parallelism, and every SWN_* variable that is set.  bench.py prints it in its line's `config`;
        tests/test_fullsize_gpu.py pins the default set."""
        sel = dict(self._kernel_sel)
        sel["wgrad_overlap"] = bool(self.overlap)
        sel["expert_parallel"] = int(self.ep.world) if self.ep is not None else 0
        sel["env_overrides"] = dict(self._env_overrides)          # (the SWN_* variables that were set when the model was built)
        return sel

    def set_kernel_switches(self, **kw):
        """Change kernel-selection switches of this model (names: resolve_kernel_switches); returns the previous values of the ones
        changed.  Takes effect with the next forward; compute copies a newly selected kernel needs are packed on demand."""
        prev = {}
        for k, v in kw.items():
            if k not in self.sw:
                raise KeyError(f"unknown kernel switch {k!r} (known: {sorted(self.sw)})")
            if self.affine and k in ("fused_heads", "fused_tail", "fused_tail_bwd") and v:
                raise ValueError(f"kernel switch {k!r}: an affine_appearance model runs the heads as their own launches (the fused tail "
                                 "does not apply the colour transform)")
            if self.sh_deg is not None and k in ("fused_heads", "fused_tail", "fused_tail_bwd") and v:
                raise ValueError(f"kernel switch {k!r}: an sh_deg model runs the heads as their own launches (the fused tail keeps its "
                                 "3-row colour head)")
            prev[k] = self.sw[k]
            self.sw[k] = type(self.sw[k])(v)
        if "overlap" in kw:
            self.overlap = self.sw["overlap"]
        return prev

    DEFAULT_KERNEL_SET = dict(geom=7, front_geom=7, tail_fused=True, fused_backward=True, comb_dwsig=True, wgrad_overlap=True)

    def _front_big(self) -> bool:
        """The dense front chains (PE -> xyz -> gate MLP, and their backward) on the persistent 256-row geometry: 256-feature layers over
        a 128-feature encoding in a 16-bit compute dtype (building.yaml).  SWN_FRONT_GEOM=1 keeps them on the 64-row kernels."""
        return ("xyz.w" in self.spec and self.M == 256 and self.G == 256 and self.KP == 128 and self.dtype != torch.float32
                and self.hash is None and self.sw["front_geom"] != 1)

    def _tail_big(self) -> bool:
        """The tail backward chain (dh2 -> dh1 -> dy with the combine backward in its write-out) on the persistent 256-row geometry:
        built and bit-exact (tests/test_kernels_gpu.py::test_chain_fused_combine_backward), but OFF by default - measured 0.23 ms per
        step SLOWER than the 64-row kernel (14.42 against 14.19 ms on one box): a two-layer chain is 5 phases, and the staging phase
        with the combine backward in it (three more operand streams behind the write-out) is the longest of them.  SWN_TAIL_GEOM=7
        turns it on (profiles/r04_experiments.md)."""
        return ("l2h.w" in self.spec and "l1.w" in self.spec and self.M == 256 and self.H2 == 128 and self.dtype != torch.float32
                and self.sw["tail_geom"] in (6, 7))

    def _tail_fused(self) -> bool:
        """The dense tail (gate scaling + ReLU, Linear "1", Linear "2" + per-ray bias, sigma / colour heads) inside the expert forward
        launch (swn_chain_desc.tail_first, chain_big.hip tag 7): 256-feature experts, 128-feature layer "2", 16-bit compute dtype,
        experts local.  SWN_FUSED_TAIL=0 keeps the 64-row tail chain as its own launch."""
        return ("l2h.w" in self.spec and "l1.w" in self.spec and self.M == 256 and self.H2 == 128 and self.dtype != torch.float32
                and self.sw["fused_heads"] and self.L + 2 <= 12 and self.sw["fused_tail"])

    def capacity(self, seg_tokens: int) -> int:
        """Rows per (segment, expert) group of a routing segment of seg_tokens points (tutel_fast_dispatch.py:210-216, top-1):
          cf > 0: int(cf * ceil(P / E)), the tokens past it are dropped;
          cf < 0: the reference's min(max(loc) + 1, int(-cf * ceil(P / E))).  Every loc is at most max(loc), so a token is kept
                  (loc < capacity) iff loc < int(-cf * ceil(P / E)): the same outputs as that static capacity (the cross-rank MAX of the
                  reference only makes max(loc) + 1 larger; only its padded buffer's size differs) - used as is, expert parallelism
                  included;
          cf = 0: max(loc) + 1, every token kept: seg_tokens, a capacity no group exceeds (the training step then runs on the packed
                  row space, one row per token - _route)."""
        if self.cf == 0:
            return int(seg_tokens)
        return int(abs(self.cf) * ((int(seg_tokens) + self.E - 1) // self.E))      # tutel_fast_dispatch.py:211 / :216

    def set_expert_parallel(self, ep):
        """Shard the experts over the ranks of `ep` (parallel.ExpertParallel) and exchange the dispatched rows instead of
        computing every expert locally.  Ownership is sharded like the reference's (models/nerf_moe.py:139, 1037-1039: expert
        parameters are kept out of DDP): a rank computes the gradients of ITS experts from the rows of all ranks, only the dense
        prefix of the flat gradient buffer is all-reduced, and Adam moves only the owner's copy of an expert (the other ranks'
        copies see an exactly-zero gradient: their weights and moments never change and are never read).  The buffers keep
        their full size (3.7 M expert parameters); gather_expert_shards() refreshes every rank's copy from the owners before a
        checkpoint / evaluation without expert parallelism."""
        assert ep is None or ep.E == self.E
        if ep is not None and self.affine:
            raise NotImplementedError("affine_appearance is not built for expert parallelism (ExpertParallel, owner_tail included): the "
                                      "colour transform runs in the local tail only")
        if ep is not None and self.cf == 0:
            raise ValueError(DYNCAP_EP_ERROR)
        if ep is not None and getattr(ep, "owner_tail", False) and self.accum_steps > 1:
            raise NotImplementedError(ACCUM_OWNER_TAIL_ERROR)
        if ep is not None and getattr(ep, "owner_tail", False) and self.check_finite:
            raise NotImplementedError(CHECK_FINITE_OWNER_TAIL_ERROR)
        if ep is None and self.ep is not None:       # leaving expert parallelism: every rank needs every expert's trained weights
            self.gather_expert_shards()
        self.ep = ep

    def gather_expert_shards(self, include_optimizer=True):
        """Every expert's parameters (and Adam moments) from its owner rank to all ranks (expert-parallel runs only): called by
        checkpoint.save_checkpoint and before leaving expert parallelism, so a checkpoint written by ANY rank holds every expert's
        trained weights.  The expert block is the contiguous tail of the flat buffers: per buffer, the owners' slices are packed
        rank-major, exchanged with ONE all_gather, and scattered back per tensor."""
        import torch.distributed as dist
        ep = self.ep
        if ep is None or ep.local:
            return
        W, El, r = ep.world, ep.El, ep.rank
        bufs = [self.flat] + ([self.m, self.v] if include_optimizer else [])
        spans = []                                   # (offset of the tensor in the flat buffer, elements per expert)
        for name, _shape in self._expert_spec:
            off, shape = self.spec[name]
            spans.append((off, int(np.prod(shape)) // self.E))
        per_rank = sum(El * per for _o, per in spans)
        for b in bufs:
            mine = torch.cat([b[off + r * El * per: off + (r + 1) * El * per] for off, per in spans])
            parts = [torch.empty_like(mine) for _ in range(W)]
            dist.all_gather(parts, mine, group=ep.group)       # (the list form: every backend implements it, gloo included)
            full = torch.stack(parts, 0)
            q = 0
            for off, per in spans:
                b[off: off + self.E * per].view(W, El * per).copy_(full[:, q:q + El * per])
                q += El * per
        self.refresh_compute_copies()

    def _local_experts(self, t, per_expert_leading=True):
        """Slice of a per-expert tensor / packed weight stream that belongs to this rank's experts."""
        if self.ep is None:
            return t
        El, r = self.ep.El, self.ep.rank
        if t.dim() == 1:                     # packed weights: [E * per]
            per = t.numel() // self.E
            v = t[r * El * per:(r + 1) * El * per]
            v.swn_nk = t.swn_nk
            return v
        return t[r * El:(r + 1) * El]

    # ------------------------------------------------------------------------------------------ buffers
    affine = False          # cfg["affine_appearance"]: the per-image affine colour transform (set by _configure)
    sh_deg = None           # cfg["sh_deg"]: spherical-harmonics colour of that degree (DenseNeRF only; set by its _configure)
    hash = None             # multiresolution hash-grid input encoding (cfg["hash"]) or None
    _grow_bufs = False      # True: one buffer per name, grown to the largest row count seen (row counts that vary per step)

    def _buf(self, name, shape, dtype):
        if self._grow_bufs:
            key = (name, tuple(shape[1:]), dtype)
            b = self._bufs.get(key)
            if b is None or b.shape[0] < shape[0]:
                b = torch.empty(shape, dtype=dtype, device=self.dev)
                self._bufs[key] = b
            return b[: shape[0]]
        key = (name, tuple(shape), dtype)
        b = self._bufs.get(key)
        if b is None:
            b = torch.empty(shape, dtype=dtype, device=self.dev)
            self._bufs[key] = b
        return b

    def _cbuf(self, c, name, shape, dtype):
        """The buffer `name` of context c's pass (tag)."""
        return self._buf(c["tag"] + ":" + name, shape, dtype)

    def _linspace(self, n):
        """torch.linspace(0, 1, n) computed on the host like the reference's CPU path, cached on the device (no host-to-device copy
        inside a step: a copy from pageable memory cannot be captured into a hipGraph)."""
        key = ("linspace", int(n))
        t = self._bufs.get(key)
        if t is None:
            t = torch.linspace(0, 1, int(n), dtype=torch.float32).to(self.dev)
            self._bufs[key] = t
        return t

    # ------------------------------------------------------------------------------------------ forward
    def forward_rays(self, rays, image_indices, n_samples, seg_tokens, perturb=0.0, perturb_rand=None, sigma_noise=None,
                     training=True, routing_override=None, no_batch=False, z_in=None, pe_dir=None, tag="c",
                     want_weights=False, composite=True, sigma_noise_std=0.0, head=None):
        """One pass of render_rays' _inference (rendering.py:277-494) over N rays x n_samples points: sampling (or the
        caller's depths z_in for the fine pass), positional encoding, the network, and (optionally) compositing.
        Returns a context dict holding every tensor the backward needs and the rendered results.
        Device noise on (set_device_noise) and a training pass: the jitter (perturb > 0, no perturb_rand) and the sigma noise
        (sigma_noise_std > 0, no sigma_noise) are drawn from the seeded generator; supplied tensors win."""
        o, dt, dev = ops, self.dtype, self.dev
        N, S = rays.shape[0], n_samples
        self._sync_compute_copies()       # (an optimizer outside this class may have stepped flat_param since the last forward)
        dn = self.noise if training and self.noise.on else None
        jitter_rng = dn is not None and perturb > 0 and perturb_rand is None and z_in is None
        drawn = None
        if dn is not None and sigma_noise is None and sigma_noise_std > 0:
            sigma_noise = drawn = dn.draw(o.RNG_SIGMA if tag == "c" else o.RNG_SIGMA_FINE, N * S, dn.base * S, o.RNG_NORMAL,
                                          float(sigma_noise_std))
        if jitter_rng and self.hash is not None:      # (the plain path draws it inside swn_sample_pe_rng)
            perturb_rand = dn.draw(o.RNG_JITTER, N * S, dn.base * S, o.RNG_UNIFORM).view(N, S)
        if self.hash is not None:         # hash-grid encoding of the sample positions (BASELINE configs[4])
            z = z_in if z_in is not None else o.sample_z(rays, self._linspace(S), perturb_rand,
                                                         perturb, S)
            pe = o.hash_encode_fwd(rays, z, self.p["hash.table"], self.hash, dt, self.KP)
            if pe_dir is None:
                pe_dir = self._dir_pe(rays)
        elif z_in is None:
            t_steps = self._linspace(S)
            if jitter_rng:
                z, pe, pe_dir = o.sample_pe_rng(rays, t_steps, dn.seed, dn.step, dn.base, perturb, S,
                                                self.cfg["pos_xyz_dim"], self.cfg["pos_dir_dim"], dt, self.KP, self.DP)
            else:
                z, pe, pe_dir = o.sample_pe(rays, t_steps, perturb_rand, perturb, S, self.cfg["pos_xyz_dim"],
                                            self.cfg["pos_dir_dim"], dt, self.KP, self.DP)
        else:
            z = z_in
            pe = o.pe_from_z(rays, z_in, self.cfg["pos_xyz_dim"], dt, self.KP)      # xyz_fine_fn, rendering.py:103
            if pe_dir is None:
                pe_dir = self._dir_pe(rays)
        # (an inference pass saves no activations / ReLU masks: nothing will run backward)
        c = self._net_forward(pe, pe_dir, image_indices, N, S, seg_tokens, sigma_noise, routing_override, no_batch, tag,
                              saving=bool(training), head=head)
        c["z"], c["rays"] = z, rays
        if drawn is not None:
            c["sigma_noise"] = drawn          # (the draw of this pass, for inspection; a supplied tensor is the caller's)
        if composite:
            c["rgb"], c["depth"], c["depth_variance"], c["weights"] = o.composite_fwd(c["raw"], c["z"], want_weights=want_weights)
        return c

    # ------------------------------------------------------------------------------------------ seeded device noise
    def set_device_noise(self, seed, step: int = 0, ray_base: int = 0):
        """Seeded device-side noise (csrc/philox.hpp): seed = None turns it off (the default - nothing differs from a model that never
        called this).  On: a TRAINING forward draws what the caller does not supply - the stratified jitter (perturb > 0), the sigma
        noise (sigma_noise_std > 0), the fine pass's u and the gate noise - from Philox4x32-10 keyed by (seed, step, stream, global
        element index), ray i of this call being global ray ray_base + i.  The draw is a pure function of those four: identical in eager
        mode and in a captured graph, on one GPU and on W GPUs (ray_base = the rank's first global ray), and after a resume
        (noise_state_dict).  The step lives on the device and is advanced by the last launch of every training step.
        (A graph captured earlier keeps the seed and ray_base it was captured with; the step it reads from the device.)"""
        self.noise.set(seed, step, ray_base, self.dev)

    @property
    def device_noise(self) -> bool:
        return self.noise.on

    def set_ray_base(self, ray_base: int):
        """The global index of this model's first ray (data parallel: the rank's slice of the batch, parallel.shard_rays).  Set before
        the noise is switched on through hparams.device_noise_seed (rendering.render_rays), it is what that switch-on starts with."""
        self.noise.set_base(ray_base)

    def noise_state_dict(self) -> dict:
        """{"seed", "step", "ray_base"} - what a resume needs besides the parameters (seed None: device noise off).  Reads the step
        back from the device.  Store it next to a checkpoint, e.g. torch.save({**ckpt, "noise_state": model.noise_state_dict()})."""
        return self.noise.state_dict()

    def load_noise_state_dict(self, sd: dict):
        self.set_device_noise(sd.get("seed"), int(sd.get("step", 0)), int(sd.get("ray_base", 0)))

    def _noise_advance(self):
        """The step counter's advance: the LAST launch of a training step (inside a captured step).  Nothing with device noise off."""
        self.noise.advance()

    def _dir_pe(self, rays):
        """PE of the ray directions only (per ray)."""
        N = rays.shape[0]
        l_xyz = 0 if self.hash is not None else self.cfg["pos_xyz_dim"]      # (the position encoding of this call is discarded)
        _, _, pe_dir = ops.sample_pe(rays, torch.zeros(1, device=self.dev), None, 0.0, 1, l_xyz,
                                     self.cfg["pos_dir_dim"], self.dtype, self.KP, self.DP)
        return pe_dir

    def _net_forward(self, pe, pe_dir, image_indices, N, S, seg_tokens, sigma_noise, routing_override, no_batch, tag, *, saving, head=None):
        """NeRFMoE.forward over the N*S points whose encodings are in `pe`, evaluated in model chunks of seg_tokens points like
        the reference's loop (rendering.py:354-383): routing, capacity and l_aux are per chunk.  A ragged last chunk
        (N*S not a multiple of seg_tokens) is routed on its own with its own capacity, exactly as the reference does - in
        evaluation and in training (backward_net walks the two parts).
        saving: a training pass (the chains save activations and ReLU masks); head: None for the model's own heads, or a ShHead /
        CoefHead record (DenseNeRF).  Both travel in the context (c["saving"], c["head"]), where every phase reads them."""
        mode = dict(saving=saving, head=head)
        P = N * S
        seg_tokens = min(seg_tokens, P)
        if P % seg_tokens == 0:
            return self._net_forward_rows(pe, pe_dir, image_indices, N, S, seg_tokens, sigma_noise, routing_override, no_batch, tag, None, **mode)
        main = (P // seg_tokens) * seg_tokens
        a = self._net_forward_rows(pe, pe_dir, image_indices, N, S, seg_tokens, sigma_noise, routing_override, no_batch, tag, (0, main), **mode)
        b = self._net_forward_rows(pe, pe_dir, image_indices, N, S, P - main, sigma_noise, routing_override, no_batch, tag + "t", (main, P), **mode)
        c = dict(N=N, S=S, P=P, n_seg=a["n_seg"] + 1, seg_tokens=seg_tokens, tag=tag, image_indices=image_indices, ragged=True,
                 parts=(a, b), pe=pe, pe_dir=pe_dir)
        for k in ("raw", "l_aux", "idx", "gmax"):
            c[k] = torch.cat([a[k], b[k]], 0)
        return c

    def _join_side_outputs(self, ev, *tensors):
        """The launch stream waits for work issued on the side stream.  Allocation invariant: tensors allocated on the side
        stream (ray_feat, c_ray) are consumed on the launch stream, tensors allocated on the launch stream (dc_ray, dh2, dsig in
        backward_net_a) are read on the side stream - safe because EVERY side-stream section starts with side.wait_event(<launch-stream
        event>) and ends in an event the launch stream waits for before the tensors' last use, and the readers' inputs are kept alive in the
        returned state until that join: no block can be handed to the other stream's allocations while it is still in use.
        (`Tensor.record_stream` is deliberately NOT used: these tensors live in a captured graph's private pool - blocks with recorded
        streams are freed through deferred events when the graph is dropped; a bench.py run that creates and drops two graphed steps died
        with SIGSEGV once in a while with it, round 6.)"""
        torch.cuda.current_stream().wait_event(ev)
        if _EXP_RECORD_STREAM:      # (experiment only: scripts/experiments/graph_drop_stress.py reproduces the crash with it)
            for t in tensors:
                if t is not None and t.is_cuda:
                    t.record_stream(torch.cuda.current_stream())

    def _on_side(self, fn):
        """fn() on the side stream, behind an event recorded on the launch stream now; returns the event that marks its completion."""
        # (the shape of EVERY side-stream section: _join_side_outputs.  What fn allocates is allocated on the side stream.)
        ready = torch.cuda.Event()
        ready.record()
        with torch.cuda.stream(self.side):
            self.side.wait_event(ready)
            fn()
            done = torch.cuda.Event()
            done.record()
        return done

    def _ray_feat(self, c, pe_dir, image_indices):
        """The per-ray part of layer "2": [PE(dir), appearance embedding] @ W2r + b2 (N_rays x 75) -> c["ray_feat"], c["c_ray"]."""
        # (one launch: swn_ray_feat_fwd - was cat / embedding lookup / addmm in torch)
        if self.affine:      # the direction encoding only; the embedding goes through affine -> the per-ray 3 x 4 colour transform
            idx = image_indices.contiguous()
            c["ray_feat"], c["c_ray"] = ops.ray_feat_dir_fwd(pe_dir, self.in_dir, self.p["emb"], idx, self.p["l2r.w"], self.p["l2.b"])
            c["aff_T"] = ops.affine_ray_fwd(self.p["emb"], idx, self.p["affine.w"], self.p["affine.b"])
            return
        c["ray_feat"], c["c_ray"] = ops.ray_feat_fwd(pe_dir, self.in_dir, self.p["emb"], image_indices.contiguous(), self.p["l2r.w"], self.p["l2.b"])

    def _l2h_pad(self, forward: bool):
        """Layer "2" (256 -> 128) zero-padded to 256 (outputs of the forward copy, K of the backward-data copy) for the fused launches."""
        # (packed here when the fused kernels were switched on after the compute copies were made; refresh_compute_copies keeps it current)
        d = self.wf if forward else self.wb
        if "l2h_pad" not in d:
            d["l2h_pad"] = ops.pack_weights_padded(self.p["l2h.w"].unsqueeze(0), self.dtype, forward, 0, 256)
        return d["l2h_pad"]

    def _heads_fused(self) -> bool:
        """The sigma / colour heads inside the tail forward chain's launch (swn.h: heads_raw): rows of at most 1 KiB."""
        return self.sw["fused_heads"] and self.M in (256, 512) and self.H2 in (128, 256) and self.M * c_esz(self.dtype) <= 1024

    def _group_args(self, c, gather=True):
        """The local experts' (segment, expert) groups of the row space as launch arguments (rows gathered through the routing permutation)."""
        kw = dict(n_groups=c["ng"], n_wsets=self.E, group_stride=c["cap"], group_rows=c["counts_flat"], group_rows_clamp=c["cap"])
        if gather:
            kw["x_gather"] = c["perm"].view(-1)
        return kw

    def _net_forward_rows(self, pe, pe_dir, image_indices, N, S, seg_tokens, sigma_noise, routing_override, no_batch, tag, row_range, *, saving,
                          head=None):
        """One or more whole model chunks: front chain, gate, routing, expert chain, tail chain, heads -> c["raw"] [P, 4].
        row_range = None: all N*S points; (r0, r1): that row range of the ray-major point grid (ragged evaluation)."""
        # The driver of the forward phases: _front_forward, _route (every row-space key of the context), _expert_forward_layers, ONE
        # _experts_forward_* (the mode is chosen here), _tail_forward.
        P = N * S
        if row_range is not None:
            r0, r1 = row_range
            P = r1 - r0
            pe = pe[r0:r1]
            sigma_noise = None if sigma_noise is None else sigma_noise[r0:r1]
            routing_override = None if routing_override is None else routing_override[r0:r1]
        assert P % seg_tokens == 0, "points must be a multiple of the segment (model chunk) size"
        # tutel_fast_dispatch.py:210-216; eval path (apply_on_expert_fn_nobatch): nothing is dropped == a capacity nothing exceeds
        cap = seg_tokens if no_batch else self.capacity(seg_tokens)
        if self.cf == 0 and not no_batch and self.ep is not None:
            raise ValueError(DYNCAP_EP_ERROR)
        c = dict(N=N, S=S, P=P, n_seg=P // seg_tokens, cap=cap, seg_tokens=seg_tokens, tag=tag, image_indices=image_indices,
                 saving=bool(saving), head=head)
        c["pe"], c["pe_dir"] = pe, pe_dir
        # the per-ray half of layer "2" (gather + a 75 x 128 GEMM per ray: one small launch) only needs the direction encoding: on the side
        # stream it runs under the front chain / the router instead of between the routing and the expert launch
        ray_feat_ev = None
        if (self.overlap and self.side is not None and not self.profile and self.ep is None and row_range is None and self._tail_fused()
                and "l2r.w" in self.p):
            ray_feat_ev = self._on_side(lambda: self._ray_feat(c, pe_dir, image_indices))
        gnoise = self._front_forward(c, N, row_range)
        owner = self._route(c, gnoise, routing_override, no_batch, row_range)
        layers = self._expert_forward_layers(c)
        # ---- the expert chain (gathers its rows through perm; ragged groups = (segment, expert)): ONE mode per forward
        if no_batch and not c["saving"] and self.ep is not None:
            self._experts_forward_ep_nobatch(c, layers)
        elif self.ep is None and c["tail_fused"]:
            return self._experts_forward_fused(c, layers, pe_dir, image_indices, sigma_noise, ray_feat_ev)
        elif self.ep is None:
            self._experts_forward_local(c, layers)
        elif owner:
            from . import ep_owner
            return ep_owner.forward(self, c, layers, pe_dir, image_indices, sigma_noise, c["saving"])
        else:
            self._experts_forward_ep(c, layers)
        # ---- per-ray part of layer "2"
        if ray_feat_ev is not None:        # (issued on the side stream above; this branch: the fused tail was not taken after all)
            self._join_side_outputs(ray_feat_ev, c["ray_feat"], c["c_ray"])
        else:
            self._ray_feat(c, pe_dir, image_indices)
        rowbias, rpb = c["c_ray"], S
        if row_range is not None:  # a row range of the point grid: the rows' rays through an explicit per-row gather
            rowbias, rpb = c["c_ray"].index_select(0, torch.arange(r0, r1, device=self.dev) // S), 1
            c["ragged"], c["row0"] = True, r0
        if self.affine:      # the heads' view of the per-ray transform: one matrix per S rows, or (a row range) per row
            c["aff_rows"] = (c["aff_T"], S) if row_range is None else (c["aff_T"].index_select(0, torch.arange(r0, r1, device=self.dev) // S), 1)
        self._tail_forward(c, c["eo"], sigma_noise, rowbias, rpb, combine=(c["row_of_tok"], c["gmax"]))
        return c

    def _front_forward(self, c, N, row_range):
        """Front chain PE -> xyz -> gate MLP (c["h0"], c["a1"], c["g"]); returns the gate-noise draw of a training forward (or None)."""
        o, dt, dev = ops, self.dtype, self.dev
        P, S, M, G, E = c["P"], c["S"], self.M, self.G, self.E
        c["h0"] = self._cbuf(c, "h0", (P, M), dt)
        c["a1"] = self._cbuf(c, "a1", (P, G), dt)
        c["g"] = self._cbuf(c, "g", (P, G), dt)
        c["m_a1"] = self._cbuf(c, "m_a1", (o.chain_mask_words(dt, 1, P, max(M, G, self.KP)),), torch.int32)
        sv = c["saving"]
        c["no_grad"] = not sv
        # (the 64-row kernels re-stream the 320 KB of weights from L2 for every 64 rows - 11.8 GB of L2 reads per 2M-point launch against
        #  0.5 GB of input, the CU's L2 -> L1 path is what bounds them - the persistent 256-row geometry a quarter of that)
        c["front_geom"] = self.sw["front_geom"] if self._front_big() else 1
        big = c["front_geom"] >= 6
        o.mlp_chain(c["pe"], [o.Layer(self.wf["xyz_pad" if big else "xyz"], self.p["xyz.b"].view(1, M), save=c["h0"]),
                              o.Layer(self.wf["gate0"], self.p["gate0.b"].view(1, G), relu=1, mask=c["m_a1"] if sv else None,
                                      save=c["a1"] if sv else None),
                              o.Layer(self.wf["gate1"], self.p["gate1.b"].view(1, G))], c["g"], tag=3, geometry=c["front_geom"] if big else 0,
                    x_features=self.KP if big else 0, x_k=self._xyz_k() if c["front_geom"] == 7 else 0)
        if not (sv and self.gate_noise > 0):       # (training only, like `self.training and self.gate_noise > 0`)
            return None
        if self.gate_noise_draw is None and self.noise.on:     # stream 4, element (ray_base * S + point) * E + expert
            r0 = 0 if row_range is None else row_range[0]
            return self.noise.draw(o.RNG_GATE, P * E, (self.noise.base * S + r0) * E, o.RNG_NORMAL).view(P, E)
        if self.gate_noise_draw is None:
            return torch.randn(P, E, device=dev, dtype=torch.float32)
        # a supplied draw (tests): [N * S, E] of this pass's point grid; a row range takes its rows
        draw = self.gate_noise_draw.to(dev, torch.float32)
        if draw.numel() != N * S * E:
            raise ValueError(f"gate_noise_draw holds {draw.numel()} values, this pass needs [{N * S}, {E}] (one row per point)")
        draw = draw.reshape(N * S, E)
        return (draw if row_range is None else draw[row_range[0]:row_range[1]]).contiguous()

    def _route(self, c, gnoise, routing_override, no_batch, row_range):
        """Gate, routing override, the packed / dyn / want_drops decisions, routing; returns whether the step hands over to ep_owner.py."""
        # Fills EVERY row-space key of the context: idx, gmax, geom, tail_fused, dyn, loc, counts, perm, tok2row, l_aux, drop_begin / dropped,
        # group_begin, packed_rows, rows, ng, counts_flat.
        o, dt, dev, sv = ops, self.dtype, self.dev, c["saving"]
        P, n_seg, cap, seg_tokens, M, E = c["P"], c["n_seg"], c["cap"], c["seg_tokens"], self.M, self.E
        c["gates"], c["idx"], c["gmax"], c["stats"] = o.gate_fwd(c["g"], self.p["ln.w"], self.p["ln.b"], self.p["wg"], noise=gnoise,
                                                                 noise_scale=self.gate_noise / E)
        if routing_override is not None:     # tests: inject the oracle's expert choice (near-tie robustness)
            c["idx"] = routing_override.to(dev).int().contiguous()
            c["gmax"] = c["gates"].gather(1, c["idx"].long()[:, None])[:, 0].contiguous()
        # capacity_factor = 0 (the reference's dynamic capacity: nothing dropped) outside the no-batch forms: the packed row space, one row
        # per token (the strided one would hold n_seg * E * seg_tokens rows - E times the saves, masks and perm)
        dyn = c["dyn"] = self.cf == 0 and not no_batch
        packed = (bool(no_batch) and not sv and self.ep is None) or dyn      # (see below: the packed row layout)
        # expert chains (forward here, backward-data in backward_net - the pair shares its ReLU mask layout): the 256-row geometry
        # with phase-shifted row groups as a persistent launch (chain_big.hip, geometry 7 = geometry 4 walking a tile queue) for 256-feature
        # experts in a 16-bit compute dtype once a group holds at least one full tile.  The chain_geom switch picks another one (1: the
        # 64-row kernels, 2 / 4 / 5 / 6: see include/swn.h) - tests.
        c["geom"] = o.expert_geometry(M, dt, cap, self.sw["chain_geom"])
        # the tail inside the expert launch (local experts, standard row space, whole point grid): the expert output never reaches memory
        c["tail_fused"] = (self._tail_fused() and self.ep is None and c["geom"] == 7 and row_range is None
                           and P * M * c_esz(dt) < (1 << 32) - 64)
        # expert parallelism with the tail on the expert's rank (ep_owner.py): the same fused launches, on a received token space
        from . import ep_owner
        owner = ep_owner.eligible(self, c, no_batch, row_range)
        # (the fused tail's list of dropped tokens comes out of the routing launch)
        want_drops = (c["tail_fused"] or owner) and not packed
        if dyn:     # the routing writes the packed row space itself (no strided perm, no pack pass); nothing is dropped
            c["loc"], c["counts"], c["group_begin"], c["perm"], c["tok2row"], c["l_aux"] = o.route_top1_packed(c["idx"], c["gmax"], c["gates"],
                                                                                                             seg_tokens, E, self.bpr)
            if c["tail_fused"]:      # the fused tail's (empty) list of dropped tokens: a zero count, never written
                key = ("dyn_nodrops", n_seg * E)
                if key not in self._bufs:
                    self._bufs[key] = (torch.zeros(n_seg * E + 1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev))
                c["drop_begin"], c["dropped"] = self._bufs[key]
        else:
            routed = o.route_top1(c["idx"], c["gmax"], c["gates"], seg_tokens, E, cap, self.bpr, want_perm=not packed, want_drops=want_drops)
            c["loc"], c["counts"], c["perm"], c["tok2row"], c["l_aux"] = routed[:5]
            if want_drops:
                c["drop_begin"], c["dropped"] = routed[5], routed[6]
        # evaluation without token dropping (apply_on_expert_fn_nobatch, tutel_moe_layer_nobatch.py:237-352): the reference packs the
        # rows contiguously per expert (expert_locations_begin, tutel_fast_dispatch_nobatch.py:24-36).  Same layout here for the
        # inference forward: P rows instead of n_seg * E * seg_tokens, groups addressed through their first row.
        if packed and not dyn:
            c["group_begin"], c["perm"], c["tok2row"] = o.route_pack(c["idx"], c["loc"], c["counts"], seg_tokens, E)
        # packed ReLU-mask slots (swn_chain_desc.packed_rows) in the no-drop row space: the masks follow the P rows too (and the persistent
        # launch walks P / 256 + groups tiles instead of groups * seg_tokens / 256; an inference forward on another geometry: no masks)
        c["packed_rows"] = P if (dyn and (sv or c["geom"] in (0, 1, 7))) else 0
        c["rows"], c["ng"] = P if packed else n_seg * E * cap, n_seg * E
        c["counts_flat"] = c["counts"].view(-1)
        return owner

    def _expert_forward_layers(self, c):
        """The expert chain's save / mask / output buffers of the context's row space and its forward layer list (this rank's experts)."""
        o, dt, sv, L, M = ops, self.dtype, c["saving"], self.L, self.M
        P, n_seg, cap, rows, ng = c["P"], c["n_seg"], c["cap"], c["rows"], c["ng"]
        c["saves"] = [self._cbuf(c, f"save{l}", (rows, M), dt) if sv else None for l in range(L - 1)]
        if c["packed_rows"]:
            nw = o.chain_mask_words_packed(dt, P, ng, M)
        else:
            nw = max(o.chain_mask_words(dt, ng, cap, M), n_seg * o.chain_mask_words(dt, self.E, cap, M))    # (expert parallel: one launch per segment)
        c["masks"] = [self._cbuf(c, f"mask{l}", (nw,), torch.int32) if sv else None for l in range(L - 1)]
        c["eo"] = None if c["tail_fused"] else self._cbuf(c, "eo", (rows, M), dt)
        self._kernel_sel.update(geom=c["geom"], front_geom=c["front_geom"], tail_fused=bool(c["tail_fused"]))
        return o.expert_fwd_layers([self._local_experts(self.wf[f"exp{l}"]) for l in range(L)],
                                   [self._local_experts(self.p[f"exp{l}.b"]) for l in range(L)], set(self.cfg["skips"]), c["saves"], c["masks"])

    def _experts_forward_ep_nobatch(self, c, layers):
        """Expert-parallel evaluation without token dropping, segment by segment, into c["eo"] (packed rows)."""
        # evaluation without token dropping under expert parallelism (tutel_moe_layer_nobatch.py:308-335): the packed rows of a
        # segment, expert-major = (destination rank, local expert), travel with UNEQUAL splits (the reference's list_all_to_all);
        # the owner runs its experts on the (source rank, local expert) groups it received and sends the rows back
        o, ep, seg_tokens = ops, self.ep, c["seg_tokens"]
        _gb, perm_p, c["tok2row"] = o.route_pack(c["idx"], c["loc"], c["counts"], seg_tokens, self.E)
        c["row_of_tok"] = c["tok2row"]
        c["eo"] = self._buf(c["tag"] + ":eo_packed", (c["P"], self.M), self.dtype)
        for s_ in range(c["n_seg"]):
            rs = slice(s_ * seg_tokens, (s_ + 1) * seg_tokens)          # every segment holds exactly seg_tokens packed rows
            recv, rc = ep.all_to_all_ragged(o.gather_rows(c["h0"], perm_p[rs]), c["counts"][s_].contiguous())
            out = torch.empty_like(recv)
            if recv.shape[0]:
                gb = (torch.cumsum(rc, 0) - rc).to(torch.int32)
                o.mlp_chain(recv, layers, out, n_groups=ep.world * ep.El, n_wsets=ep.El, group_stride=seg_tokens, group_rows=rc,
                            group_rows_clamp=seg_tokens, tag=1, geometry=c["geom"], group_begin=gb)
            back, _ = ep.all_to_all_ragged(out, rc, recv_counts=c["counts"][s_].contiguous())
            c["eo"][rs] = back

    def _experts_forward_fused(self, c, layers, pe_dir, image_indices, sigma_noise, ray_feat_ev):
        """Local experts + tail + heads in ONE launch -> c["raw"]; returns the finished context."""
        # ---- experts + tail in ONE launch (chain_big.hip, tag 7): behind the last expert layer a row is scaled by its gate value and
        # ReLU'd (the decoded MoE output y), runs through layer "1" and layer "2" (+ the per-ray bias below) and the two heads; y, h1
        # and h2 are saved in TOKEN order for the backward (a training forward), raw is written in token order; the tokens no expert
        # kept enter at layer "1" as zero rows (swn_route_dropped).  Replaces: the expert output's round trip through memory, the
        # 64-row tail chain (which re-streams its 192 KiB of weights from L2 for every 64 rows) and its launch.
        o, dt, sv = ops, self.dtype, c["saving"]
        P, S, M, H2, L = c["P"], c["S"], self.M, self.H2, self.L
        c["row_of_tok"] = c["tok2row"]
        if ray_feat_ev is not None:
            self._join_side_outputs(ray_feat_ev, c["ray_feat"], c["c_ray"])
        else:
            self._ray_feat(c, pe_dir, image_indices)
        if "dropped" not in c:
            c["drop_begin"], c["dropped"] = o.route_dropped(c["idx"], c["loc"], c["counts"], c["seg_tokens"], self.E, c["cap"])
        w2 = self._l2h_pad(True)
        c["y"] = self._cbuf(c, "y", (P, M), dt) if sv else None
        c["h1"] = self._cbuf(c, "h1", (P, M), dt) if sv else None
        c["h2"] = self._cbuf(c, "h2", (P, H2), dt) if sv else None
        c["raw"] = torch.empty(P, 4, dtype=torch.float32, device=self.dev)
        heads = (self.p["sigma.w"], self.p["sigma.b"], self.p["color.w"], self.p["color.b"], sigma_noise, c["raw"])
        last = layers[-1]
        full = layers[:-1] + [o.Layer(last.w, last.b, relu=last.relu, skip=last.skip, save=c["y"]),
                              o.Layer(self.wf["l1"], self.p["l1.b"].view(1, M), save=c["h1"]),
                              o.Layer(w2, None, relu=1, rowbias=c["c_ray"], rows_per_bias=S)]
        grp, extra = self._group_args(c), dict(group_begin=c.get("group_begin"), packed_rows=c["packed_rows"])

        def run_experts(save=sv):
            o.mlp_chain(c["h0"], full if save else [ly.without_saves() for ly in full], c["h2"] if save else None, tag=7, geometry=7,
                        heads=heads, tail=(L, c["gmax"], c["drop_begin"], c["dropped"], H2), **grp, **extra)
        with self._timed("expert_fwd"):
            run_experts()
        if self.profile:      # bench.py: the launch again on this step's live buffers, its save-free form, and the expert layers ALONE
            def expert_gemm():    # (the grouped GEMM without the tail: tag 1, into a scratch output - what round 1-3's figure measured)
                o.mlp_chain(c["h0"], [ly.without_saves() for ly in layers], self._cbuf(c, "eo_probe", (c["rows"], M), dt), tag=1, geometry=7, **grp, **extra)
            c["_relaunch"] = {"expert_fwd": run_experts, "expert_fwd_nosave": lambda: run_experts(False), "expert_gemm_nosave": expert_gemm}
        return c

    def _experts_forward_local(self, c, layers):
        """The local experts as their own launch (tag 1) into c["eo"]; the tail chain follows as a separate launch."""
        o = ops
        c["row_of_tok"] = c["tok2row"]
        grp = self._group_args(c)

        def run_experts(lys=layers):
            o.mlp_chain(c["h0"], lys, c["eo"], tag=1, geometry=c["geom"], group_begin=c.get("group_begin"), packed_rows=c["packed_rows"], **grp)
        with self._timed("expert_fwd"):
            run_experts()
        if self.profile:      # bench.py: the same launch again, back to back, on this step's live buffers (and its save-free form)
            c["_relaunch"] = {"expert_fwd": run_experts, "expert_fwd_nosave": lambda: run_experts([ly.without_saves() for ly in layers])}

    def _experts_forward_ep(self, c, layers):
        """Expert parallel, pipelined per routing segment, kept rows or padded rows, into c["eo"]."""
        # expert parallel, pipelined per routing segment (parallel.ExpertParallel), KEPT ROWS ONLY: the kept rows of segment s, packed in
        # (expert, slot) order = payload order (destination rank, local expert, slot) -> unequal-split all-to-all on the side stream ->
        # the local experts run on the (source rank, local expert) groups (first rows from a device prefix sum) -> all-to-all back into
        # the packed row space the combine gathers from.  The dispatch of segment s + 1 and the return of segment s - 1 travel while
        # the experts work on segment s.  One host read of the counts per forward pass (ExpertParallel.plan).
        o, dt, dev, ep = ops, self.dtype, self.dev, self.ep
        n_seg, cap, rows, M, E = c["n_seg"], c["cap"], c["rows"], self.M, self.E
        W, El = ep.world, ep.El
        ngs = W * El
        recv_counts = ep.exchange_counts(c["counts"], cap, self.side)()            # [n_seg, W * E_local], the expert kernels' group order
        c["ep_counts"] = recv_counts
        c["ep_padded"] = ep.use_padded(E * cap * M * c_esz(dt))
        if c["ep_padded"]:
            # the reference's layout (tutel_moe_layer_nobatch.py:157): every (expert, capacity slot) of a segment travels - empty slots
            # as zero rows - with EQUAL splits.  The row spaces are the standard ones (perm / tok2row of swn_route_top1, group g at row
            # g * cap), nothing is read on the host: the step can be captured into a hipGraph, collectives included.
            perm_p, c["row_of_tok"] = c["perm"].view(-1), c["tok2row"]
            seg_rows = E * cap
            pl = dict(in_splits=[[El * cap] * W] * n_seg, out_splits=[[El * cap] * W] * n_seg,
                      send_off=[s_ * seg_rows for s_ in range(n_seg + 1)], recv_off=[s_ * seg_rows for s_ in range(n_seg + 1)])
            key = ("ep_begin_padded", n_seg * ngs, cap)
            if key not in self._bufs:
                self._bufs[key] = (torch.arange(n_seg * ngs, device=dev, dtype=torch.int32) * cap).contiguous()
            c["ep_begin"] = self._bufs[key]
        else:
            kept = c["counts"].clamp(max=cap)
            idx_kept = torch.where(c["loc"] < cap, c["idx"], torch.full_like(c["idx"], -1))
            _gb, perm_p, c["row_of_tok"] = o.route_pack(idx_kept, c["loc"], kept, c["seg_tokens"], E)     # packed row space of this rank's rows
            pl = ep.plan(kept, recv_counts)
            flat_rc = recv_counts.reshape(-1)
            c["ep_begin"] = (torch.cumsum(flat_rc, 0, dtype=torch.int32) - flat_rc).contiguous()      # first row of every received group
        c["ep_perm"], c["ep_plan"] = perm_p, pl
        so, ro = pl["send_off"], pl["recv_off"]
        xr = self._cbuf(c, "ep_x", (rows, M), dt)                                  # received rows of all segments (also the first layer's
        send = xr if ep.local else self._cbuf(c, "ep_send_x", (rows, M), dt)         # weight-gradient operand)
        eo_r = c["eo"] if ep.local else self._cbuf(c, "ep_eo", (rows, M), dt)        # expert outputs in the received row space
        wseg = o.chain_mask_words(dt, E, cap, M)
        c["ep_mask_words"] = wseg

        def issue(s_):
            o.gather_rows(c["h0"], perm_p[so[s_]:so[s_ + 1]], send[so[s_]:so[s_ + 1]])
            return ep.all_to_all_v(send[so[s_]:so[s_ + 1]], pl["in_splits"][s_], xr[ro[s_]:ro[s_ + 1]], pl["out_splits"][s_], self.side)
        with self._timed("expert_fwd"):
            pend = issue(0)
            returns = []
            for s_ in range(n_seg):
                nxt = issue(s_ + 1) if s_ + 1 < n_seg else None
                pend()
                if ro[s_ + 1] > ro[s_]:
                    o.mlp_chain(xr, [ly.with_mask_words(s_ * wseg, (s_ + 1) * wseg) for ly in layers], eo_r, n_groups=ngs, n_wsets=El,
                                group_stride=cap, group_rows=recv_counts[s_], group_rows_clamp=cap, tag=1, geometry=c["geom"],
                                group_begin=c["ep_begin"][s_ * ngs:(s_ + 1) * ngs])
                returns.append(ep.all_to_all_v(eo_r[ro[s_]:ro[s_ + 1]], pl["out_splits"][s_], c["eo"][so[s_]:so[s_ + 1]],
                                               pl["in_splits"][s_], self.side))
                pend = nxt
            for wait in returns:
                wait()
        c["ep_x"] = xr

    def _tail_forward(self, c, x, sigma_noise, rowbias, rows_per_bias, combine=None):
        """Layer "1" -> layer "2" (+ per-ray bias) -> heads -> c["raw"] over the rows x; combine = (row_of_tok, gate): MoE form, None: dense."""
        # ---- tail chain.  (MoE form) Its input load IS the combine: rows gathered from the expert output through tok2row, scaled by
        # the gate value, ReLU'd (dropped tokens -> zero rows) and saved as y;  then layer "1" -> layer "2" (+ per-ray bias)
        # The sigma / colour heads run inside that launch (swn.h: heads_raw): sigma from the staged y tile, colour from the h2 tile.  A
        # training forward still writes y, h1 and h2 (the backward reads them); an inference forward writes nothing but raw.
        o, dt, sv, head = ops, self.dtype, c["saving"], c["head"]
        P, M, H2 = c["P"], self.M, self.H2
        fused = self._heads_fused()
        keep = sv or not fused
        kw = {}
        if combine is not None:
            c["y"] = self._cbuf(c, "y", (P, M), dt) if keep else None
            kw = dict(x_gather=combine[0], x_save=c["y"], x_scale=combine[1], x_relu=True)
        c["h1"] = self._cbuf(c, "h1", (P, M), dt) if sv else None
        c["h2"] = self._cbuf(c, "h2", (P, H2), dt) if keep else None
        c["raw"] = torch.empty(P, 4, dtype=torch.float32, device=self.dev) if fused else None
        o.mlp_chain(x, [o.Layer(self.wf["l1"], self.p["l1.b"].view(1, M), save=c["h1"] if sv else None),
                        o.Layer(self.wf["l2h"], None, relu=1, rowbias=rowbias, rows_per_bias=rows_per_bias)], c["h2"], group_stride=P, tag=4,
                    heads=(self.p["sigma.w"], self.p["sigma.b"], self.p["color.w"], self.p["color.b"], sigma_noise, c["raw"]) if fused else None,
                    **kw)
        if self.affine:    # ---- heads + the per-image colour transform (models/nerf_moe.py:436-438) as their own launch
            c["raw"] = o.heads_affine_fwd(c["y"], c["h2"], self.p["sigma.w"], self.p["sigma.b"], self.p["color.w"], self.p["color.b"],
                                          sigma_noise, *c["aff_rows"])
        elif isinstance(head, CoefHead):   # ---- a Mega-NeRF cell training with sh_deg (DenseNeRF.forward_coef): the coefficient row itself
            c["coef_rows"] = o.heads_coef_fwd(c["y"], c["h2"], self.p["sigma.w"], self.p["sigma.b"], self.p["color.w"], self.p["color.b"],
                                              sigma_noise, self.sh_deg, *head)
        elif isinstance(head, ShHead):     # ---- heads + the spherical-harmonics contraction against the ray's direction (rendering.py:344-347)
            out = o.heads_sh_fwd(c["y"], c["h2"], self.p["sigma.w"], self.p["sigma.b"], self.p["color.w"], self.p["color.b"],
                                 sigma_noise, head.dirs, rows_per_bias, self.sh_deg, want_coef=head.want_coef)
            c["raw"], c["coef"] = out if head.want_coef else (out, None)
        elif not fused:    # ---- heads as their own launch (SWN_NO_FUSED_HEADS=1: rounds 1-2)
            c["raw"] = o.heads_fwd(c["y"], c["h2"], self.p["sigma.w"], self.p["sigma.b"], self.p["color.w"], self.p["color.b"],
                                   sigma_noise)

    # ------------------------------------------------------------------------------------------ backward
    def backward(self, c, d_rgb, d_laux):
        """Accumulates parameter gradients into self.grad given dL/d rgb [N,3] and dL/d l_aux[seg] (scalar each)."""
        d_raw = ops.composite_bwd(c["raw"], c["z"], d_rgb)
        self.backward_net(c, d_raw, d_laux)

    def backward_net(self, c, d_raw, d_laux):
        """Backward of _net_forward given dL/d raw [N*S, 4] and dL/d l_aux[seg]; accumulates into self.grad.
        = backward_net_a (heads, tail, expert chain, expert weight gradients: after it the EXPERT block of the flat gradient - 93 % of
        its bytes - is final) + backward_net_b (router, front chain, dense weight gradients).  A data-parallel step replayed from
        graphs cuts there: the all-reduce of the expert block travels while the second half runs (graph.GraphedTrainStep)."""
        if c.get("parts") is not None:
            # a ragged last model chunk (rendering.py:354-383 trains any batch size): the whole chunks and the short last chunk were
            # routed as two contexts with their own capacities; each runs its own backward on its rows of dL/d raw and its chunks'
            # share of the l_aux gradient
            a, b = c["parts"]
            if self.hash is not None:      # the parts leave dL/d encoding in their rows of one [P, KP] buffer; the table's gradient is
                d_enc = self._buf(c["tag"] + ":d_enc", (c["P"], self.KP), self.dtype)       # one launch over the whole rays behind them
                a["d_enc_out"], b["d_enc_out"] = d_enc[: a["P"]], d_enc[a["P"]:]
            self.backward_net(a, d_raw[: a["P"]], d_laux[: a["n_seg"]].contiguous())
            self.backward_net(b, d_raw[a["P"]:], d_laux[a["n_seg"]:].contiguous())
            if self.hash is not None:
                ops.hash_encode_bwd(c["rays"], c["z"], d_enc, self.hash, self.g["hash.table"])
            return
        self.backward_net_b(self.backward_net_a(c, d_raw, d_laux))

    def backward_net_a(self, c, d_raw, d_laux, join_side=False):
        """First half of backward_net (see there); returns the state backward_net_b continues from.  join_side: the launch stream
        waits for the expert weight gradients before returning (they run on the side stream otherwise and are joined at the end of
        the second half)."""
        # The driver of the backward phases: _heads_backward (heads + per-ray), _tail_backward, ONE _experts_backward_* (the mode is chosen
        # here), _expert_wgrads, then the state dict.
        if c.get("no_grad"):
            raise RuntimeError("this context comes from an inference forward (training=False): nothing was saved for the backward")
        assert c.get("parts") is None, "ragged contexts go through backward_net"
        if c.get("ep_owner") is not None:      # expert parallelism with the tail on the expert's rank
            from . import ep_owner
            return ep_owner.backward_a(self, c, d_raw, d_laux)
        # the tail's two backward layers and the combine backward in FRONT of the expert backward chain, one launch (chain_big.hip, tag 8):
        # pairs with the fused forward (its list of dropped tokens); SWN_FUSED_TAIL_BWD=0 keeps the two launches
        fused_bwd = bool(c.get("tail_fused")) and self.ep is None and self.sw["fused_tail_bwd"]
        # ... which also forms the sigma head's weight gradient where it reads y anyway (swn_chain_desc.comb_dwsig): the heads' backward
        # launch then runs without y - 512 bytes per point less (SWN_FUSED_DWSIG=0: from y in the heads' launch, as before)
        fused_dws = fused_bwd and self.M == 256 and self.sw["fused_dwsig"]
        self._kernel_sel.update(fused_backward=fused_bwd, comb_dwsig=fused_dws)
        b = dict(fused_bwd=fused_bwd, fused_dws=fused_dws)
        b["dh2"], b["dsig"], b["dc_ray"], side_small = self._heads_backward(c, d_raw, None if fused_dws else c["y"])
        self._tail_backward(c, b)
        if self.ep is not None:
            w = self._experts_backward_ep(c, b)
        elif fused_bwd:
            w = self._experts_backward_fused(c, b)
        else:
            w = self._experts_backward_local(c, b)
        side_done = None
        if self.overlap and self.side is not None and not self.profile and not join_side:
            # independent of everything that follows (they only read the saved activations / dZ and write their own
            # gradient slices): run them on the side stream, join before Adam
            side_done = self._on_side(lambda: self._expert_wgrads(c, w))
        else:
            with self._timed("expert_wgrad"):
                self._expert_wgrads(c, w)
            if self.profile and "_relaunch" in c:
                c["_relaunch"]["expert_wgrad"] = lambda: self._expert_wgrads(c, w)        # (accumulates into the gradient buffer again: timing only)
        if side_small is not None and side_done is None:      # (no expert weight gradients behind it on the side stream: join here)
            torch.cuda.current_stream().wait_event(side_small)
        return dict(c=c, d_laux=d_laux, dgmax=b["dgmax"], dx=w["dx"], dout=b["dout"], returns=w["returns"], tail_jobs=b["tail_jobs"],
                    nsp=b["nsp"], side_done=side_done,
                    keep=(b["dc_ray"], b["dh2"], b["dsig"]))      # (keep: tensors the side stream reads stay allocated to the join)

    def _ray_level_grads(self, c, dc_ray):
        """The tiny per-ray GEMM's parameter gradients (layer "2"'s ray half, its bias) and the appearance embedding's, from dc_ray."""
        o, g = ops, self.g
        if dc_ray.shape[1] in (64, 128, 256) and c["ray_feat"].shape[1] <= 256:      # split over the rays + ordered reduce (one launch)
            o.ray_feat_wgrad(c["ray_feat"], dc_ray, g["l2r.w"], g["l2.b"])
        else:
            g["l2r.w"].addmm_(c["ray_feat"].t(), dc_ray)
            g["l2.b"].add_(dc_ray.sum(0))
        if self.affine:      # the embedding's only gradient path: dT -> affine's parameters, dT @ W_a -> the ordered embedding reduction
            idx = c["image_indices"].contiguous()
            o.emb_grad(o.affine_ray_bwd(c["aff_dT"], self.p["emb"], idx, self.p["affine.w"], g["affine.w"], g["affine.b"]), idx, g["emb"])
            return
        d_feat_emb = dc_ray @ self.p["l2r.w"][self.in_dir:].t()
        o.emb_grad(d_feat_emb, c["image_indices"].contiguous(), g["emb"])        # (rays added in order: torch's index_add_ uses atomics)

    def _heads_backward(self, c, d_raw, y_heads):
        """Heads backward and the per-ray gradients; returns (dh2, dsig, dc_ray, the side stream's event or None)."""
        # per-ray bias gradient (the column sums of a ray's dh2 rows: from the heads' launch) and the tiny per-ray GEMM's parameters
        o, g = ops, self.g
        N, S, P, H2 = c["N"], c["S"], c["P"], self.H2
        if self.affine:
            if c.get("ragged"):
                raise NotImplementedError("affine_appearance: the backward of a ragged last model chunk is not built (dT is summed per "
                                          "whole ray); use a batch of rays x samples that is a multiple of the model chunk")
            dh2, dsig, dc_ray, c["aff_dT"] = o.heads_affine_bwd(y_heads, c["h2"], self.p["color.w"], self.p["color.b"], c["aff_T"], c["raw"],
                                                                d_raw, g["sigma.w"], g["sigma.b"], g["color.w"], g["color.b"], rows_per_group=S)
        elif c.get("ragged"):      # a row range of the point grid: rays may be cut at either end - per-ray sums through the rows' ray index
            dh2, dsig = o.heads_bwd(y_heads, c["h2"], self.p["color.w"], c["raw"], d_raw, g["sigma.w"], g["sigma.b"], g["color.w"],
                                    g["color.b"])
            ray_of_row = torch.arange(c["row0"], c["row0"] + P, device=self.dev) // S
            dc_ray = torch.zeros(N, H2, dtype=torch.float32, device=self.dev).index_add_(0, ray_of_row, dh2.float())
        else:
            dh2, dsig, dc_ray = o.heads_bwd(y_heads, c["h2"], self.p["color.w"], c["raw"], d_raw, g["sigma.w"], g["sigma.b"], g["color.w"],
                                            g["color.b"], rows_per_group=S)
        # The per-ray work (layer "2"'s ray half and the appearance embedding: three small launches + a reduce, ~0.1 ms in which 10-30
        # workgroups hold the chip) goes to the SIDE stream: it only needs dc_ray and writes gradient slices nobody else touches, so it
        # runs under the expert backward launch that follows (whose resident workgroups pick the few late CUs up through the tile queue);
        # joined with the expert weight gradients (same stream) or at the end of this half.  SWN_NO_OVERLAP=1: on the launch stream.
        side_small = None
        if self.overlap and self.side is not None and not self.profile and not c.get("ragged") and self.ep is None:
            side_small = self._on_side(lambda: self._ray_level_grads(c, dc_ray))
        else:
            self._ray_level_grads(c, dc_ray)
        return dh2, dsig, dc_ray, side_small

    def _tail_backward(self, c, b):
        """Tail backward (fused backward: its buffers only); adds dh1, dout, dgmax, nsp and the tail's weight-gradient jobs to b."""
        # tail backward chain: dh2 -> dh1 -> dy
        # ... with the combine backward (the sigma head's rank-1 term, the ReLU mask of y, the gate gradient, the gate scaling) applied
        # in the write-out of the last layer: dy itself never reaches memory
        o, dt = ops, self.dtype
        P, M, H2, g = c["P"], self.M, self.H2, self.g
        dh2, dsig = b["dh2"], b["dsig"]
        dh1 = self._cbuf(c, "dh1", (P, M), dt)
        dout = None if b["fused_bwd"] else self._cbuf(c, "dy", (P, M), dt)
        if b["fused_bwd"]:
            dgmax = self._cbuf(c, "dgmax", (P,), torch.float32)
            self._l2h_pad(False)
        elif M * dout.element_size() <= 1024:      # (a row's 16-byte chunks must fit one wavefront: everything but fp32 rows of 512)
            dgmax = self._cbuf(c, "dgmax", (P,), torch.float32)
            tg = self.sw["tail_geom"] if self._tail_big() else 0
            o.mlp_chain(dh2, [o.Layer(self.wb["l2h_pad" if tg >= 6 else "l2h"], None, save=dh1), o.Layer(self.wb["l1"], None)], dout, tag=5,
                        combine=(c["y"], dsig, self.p["sigma.w"], c["gmax"], dgmax), geometry=tg, x_features=H2 if tg >= 6 else 0,
                        x_k=H2 if tg == 7 else 0)
        else:
            o.mlp_chain(dh2, [o.Layer(self.wb["l2h"], None, save=dh1), o.Layer(self.wb["l1"], None)], dout, tag=5)
            dout, dgmax = o.combine_bwd(dout, c["y"], dsig, self.p["sigma.w"], c["gmax"])
        b["nsp"] = max(1, min(256, P // 1024))     # row splits of the dense weight-gradient GEMMs: one workgroup per CU also at the
                                                   # per-GPU batch of an 8-GPU run (262144 points)
        b["dh1"], b["dout"], b["dgmax"] = dh1, dout, dgmax
        b["tail_jobs"] = [(c["h1"], dh2, g["l2h.w"].view(1, M, H2), None), (c["y"], dh1, g["l1.w"].view(1, M, M), g["l1.b"].view(1, M))]

    def _xyz_k(self):
        """The first front layer's real K for the persistent chain (swn_chain_desc.x_k): the encoding's width rounded up to the K step where
        the library has a K loop of that length (80 = the default 75 columns), else the padded row's 128 columns; the rest of a c["pe"]
        row is zeros."""
        k = _ceil_to(self.in_xyz, 16)
        return k if k == 80 else 128

    def _tail_wgrads_if_large(self, c, b):
        """The tail layers' weight gradients as their own launch, at the full batch only."""
        # The weight gradients of the two tail layers: at small batches (the per-GPU share of a strong-scaling run) they go out together
        # with the front layers' at the end - one balanced launch + one reduction for all five dense layers (2.39 against 2.42 ms per
        # step at 1024 rays); at the full batch two launches are faster (15.15 against 15.30 ms: the tail operands are the most recently
        # written tensors when their launch follows the tail backward directly).  Measured on one box, scripts/ab_env.sh.
        # (fused backward: dh1 comes out of the expert launch - the tail's weight gradients follow it)
        if c["P"] > (1 << 19):
            self._dense_wgrads(b["tail_jobs"], b["nsp"])
            b["tail_jobs"] = []

    def _expert_backward_layers(self, c):
        """(dz, dx, backward layer list, the skip's y_add) of the expert backward chain in the context's row space."""
        dt, L, M, rows = self.dtype, self.L, self.M, c["rows"]
        dz = [self._cbuf(c, f"dz{l}", (rows, M), dt) for l in range(L - 1)]     # dz[L-1] = dout through perm: never materialised
        dx = self._cbuf(c, "dx", (rows, M), dt)
        bl = ops.expert_bwd_layers([self._local_experts(self.wb[f"exp{l}"]) for l in range(L)], c["masks"], dz)
        skips = list(self.cfg["skips"])
        return dz, dx, bl, dz[skips[0]] if skips else None

    def _experts_backward_fused(self, c, b):
        """Tail backward + combine backward + expert backward in ONE launch (chain_big.hip, tag 8) on the local experts."""
        o, M = ops, self.M
        dz, dx, bl, y_add = self._expert_backward_layers(c)
        dz_last = self._buf(c["tag"] + ":dz_last", (c["rows"], M), self.dtype)      # the last expert layer's dZ in the row space (the combine's output)
        lys = [o.Layer(self.wb["l2h_pad"], None, save=b["dh1"]), o.Layer(self.wb["l1"], None, save=dz_last)] + bl
        dws_dst = [self.g["sigma.w"].view(-1) if b["fused_dws"] else None]
        grp = self._group_args(c)

        def run_expert_bwd():
            o.mlp_chain(b["dh2"], lys, dx, y_add=y_add, tag=8, geometry=7, x_features=self.H2, x_k=self.H2,
                        combine=(c["y"], b["dsig"], self.p["sigma.w"], c["gmax"], b["dgmax"], dws_dst[0]), head=(2, c["drop_begin"], c["dropped"]),
                        group_begin=c.get("group_begin"), packed_rows=c.get("packed_rows", 0), **grp)
        with self._timed("expert_bwd"):
            run_expert_bwd()
        if self.profile and "_relaunch" in c:
            if b["fused_dws"]:      # (a relaunch for timing adds into a scratch vector, not into the gradient)
                dws_dst[0] = torch.zeros(M, dtype=torch.float32, device=self.dev)
            c["_relaunch"]["expert_bwd"] = run_expert_bwd
        self._tail_wgrads_if_large(c, b)
        return dict(x_first=c["h0"], dz_last=dz_last, dz=dz, dx=dx, a_gather=grp["x_gather"], b_gather=None, returns=None)

    def _experts_backward_local(self, c, b):
        """The local experts' backward chain as its own launch (tag 2): dy read through the routing permutation."""
        o = ops
        self._tail_wgrads_if_large(c, b)
        dz, dx, bl, y_add = self._expert_backward_layers(c)
        grp = self._group_args(c)

        def run_expert_bwd():
            o.mlp_chain(b["dout"], bl, dx, y_add=y_add, tag=2, geometry=c["geom"], group_begin=c.get("group_begin") if c.get("packed_rows") else None,
                        packed_rows=c.get("packed_rows", 0), **grp)
        with self._timed("expert_bwd"):
            run_expert_bwd()
        if self.profile and "_relaunch" in c:
            c["_relaunch"]["expert_bwd"] = run_expert_bwd
        return dict(x_first=c["h0"], dz_last=b["dout"], dz=dz, dx=dx, a_gather=grp["x_gather"], b_gather=grp["x_gather"], returns=None)

    def _experts_backward_ep(self, c, b):
        """The expert-parallel backward chain, pipelined per routing segment."""
        # per segment like the forward pass: dispatch of segment s + 1 and return of segment s - 1 overlap the chain of segment s;
        # the input gradients come home into the packed row space (dx) that the front backward chain gathers from
        o, dt, ep = ops, self.dtype, self.ep
        n_seg, cap, rows, M, dout = c["n_seg"], c["cap"], c["rows"], self.M, b["dout"]
        pl, perm_p = c["ep_plan"], c["ep_perm"]
        so, ro = pl["send_off"], pl["recv_off"]
        dr = self._cbuf(c, "ep_d", (rows, M), dt)
        dsend = dr if ep.local else self._cbuf(c, "ep_send_d", (rows, M), dt)

        def issue_b(s_):
            o.gather_rows(dout, perm_p[so[s_]:so[s_ + 1]], dsend[so[s_]:so[s_ + 1]])
            return ep.all_to_all_v(dsend[so[s_]:so[s_ + 1]], pl["in_splits"][s_], dr[ro[s_]:ro[s_ + 1]], pl["out_splits"][s_], self.side)
        pend = issue_b(0)      # the rows of the first segment travel to their experts while the tail's weight gradients run
        self._tail_wgrads_if_large(c, b)
        dz, dx, bl, y_add = self._expert_backward_layers(c)
        ngs = ep.world * ep.El
        dx_r = dx if ep.local else self._cbuf(c, "ep_dx", (rows, M), dt)
        wseg = c["ep_mask_words"]
        returns = []
        with self._timed("expert_bwd"):
            for s_ in range(n_seg):
                nxt = issue_b(s_ + 1) if s_ + 1 < n_seg else None
                pend()
                if ro[s_ + 1] > ro[s_]:
                    o.mlp_chain(dr, [ly.with_mask_words(s_ * wseg, (s_ + 1) * wseg) for ly in bl], dx_r, n_groups=ngs, n_wsets=ep.El,
                                group_stride=cap, group_rows=c["ep_counts"][s_], group_rows_clamp=cap, y_add=y_add, tag=2, geometry=c["geom"],
                                group_begin=c["ep_begin"][s_ * ngs:(s_ + 1) * ngs])
                returns.append(ep.all_to_all_v(dx_r[ro[s_]:ro[s_ + 1]], pl["out_splits"][s_], dx[so[s_]:so[s_ + 1]], pl["in_splits"][s_],
                                               self.side))
                pend = nxt
        # the received rows, already in group order: no gather
        return dict(x_first=c["ep_x"], dz_last=dr, dz=dz, dx=dx, a_gather=None, b_gather=None, returns=returns)

    def _expert_wgrads(self, c, w):
        """Expert weight gradients from w, what the mode's _experts_backward_* returned."""
        # all layers in ONE launch: layer 0 reads its input rows, layer L-1 its dZ rows, through the routing permutation
        o, g, L, ep = ops, self.g, self.L, self.ep
        items = o.expert_wgrad_items(w["x_first"], c["saves"], w["dz"], w["dz_last"], [self._local_experts(g[f"exp{l}.w"]) for l in range(L)],
                                     [self._local_experts(g[f"exp{l}.b"]) for l in range(L)], w["a_gather"], w["b_gather"])
        grp = self._group_args(c, gather=False)
        if ep is not None:      # received rows are packed: groups through their first rows (any width: wgrad_multi cuts 512-feature
            grp.update(n_wsets=ep.El, group_rows=c["ep_counts"].reshape(-1))      # operands into 256-column GEMMs of the same launch)
            o.wgrad_multi(items, tag=1, group_begin=c["ep_begin"], **grp)
        elif c.get("packed_rows"):      # the no-drop row space (capacity_factor = 0): the same balanced launch over the packed groups -
            o.wgrad_multi(items, tag=1, group_begin=c["group_begin"], **grp)      # it cuts the valid rows into equal shares (no row-split heuristic)
        else:
            for i0 in range(0, L, 8):
                o.wgrad_batched(items[i0:i0 + 8], n_splits=self.expert_wgrad_splits or max(1, min(256 // c["ng"], c["cap"] // 2048)), tag=1, **grp)

    def backward_net_b(self, st):
        """Second half of backward_net: router backward, front backward chain, dense weight gradients (+ the hash table's)."""
        o, dt = ops, self.dtype
        c, d_laux, dgmax, dx, returns, tail_jobs, nsp, side_done = (st[k] for k in ("c", "d_laux", "dgmax", "dx", "returns", "tail_jobs",
                                                                                   "nsp", "side_done"))
        P, seg_tokens = c["P"], c["seg_tokens"]
        M, E, G = self.M, self.E, self.G
        g, ep = self.g, self.ep
        # gate backward (softmax / router / LayerNorm) including the l_aux term
        coef = (d_laux * (E / float(seg_tokens * seg_tokens))).to(torch.float32).contiguous()
        dg = o.gate_bwd(c["g"], self.p["ln.w"], self.p["ln.b"], self.p["wg"], c["gates"], c["idx"], dgmax, c["stats"],
                        c["counts"], coef, seg_tokens, g["wg"], g["ln.w"], g["ln.b"])
        # front backward chain: dg -> d(a1) -> d(h0), adding the expert path's input gradient through tok2row
        dza1 = self._cbuf(c, "dza1", (P, G), dt)
        dh0 = self._cbuf(c, "dh0", (P, M), dt)
        if ep is not None:      # (the input gradients travelled home under the expert weight gradients / the router backward)
            for wait in returns:
                wait()
        o.mlp_chain(dg, [o.Layer(self.wb["gate1"], None, relu=2, mask=c["m_a1"], save=dza1), o.Layer(self.wb["gate0"], None)],
                    dh0, y_add=dx, y_add_gather=c["row_of_tok"], tag=6, geometry=c["front_geom"] if c["front_geom"] >= 6 else 0)
        self._dense_wgrads(tail_jobs + [(c["a1"], dg, g["gate1.w"].view(1, G, G), g["gate1.b"].view(1, G)),
                                        (c["h0"], dza1, g["gate0.w"].view(1, M, G), g["gate0.b"].view(1, G)),
                                        (c["pe"], dh0, g["xyz.w"].view(1, self.KP, M), g["xyz.b"].view(1, M))], nsp)
        if self.hash is not None:          # dL/d encoding = dh0 W_xyz^T, scattered into the hash table's gradient
            d_enc = c.get("d_enc_out")     # (a part of a ragged batch: its rows of the batch's buffer - backward_net scatters them)
            part = d_enc is not None
            if not part:
                d_enc = self._cbuf(c, "d_enc", (P, self.KP), dt)
            o.mlp_chain(dh0, [o.Layer(self.wb["xyz"], None)], d_enc, tag=0)
            if not part:
                o.hash_encode_bwd(c["rays"], c["z"], d_enc, self.hash, g["hash.table"])
        if side_done is not None:
            torch.cuda.current_stream().wait_event(side_done)

    def _dense_wgrads(self, jobs, n_splits):
        """Weight gradients of dense layers that are ready together, (a, dz, dw, db) each: ONE balanced launch and one reduction
        (swn_wgrad_multi) for layers of up to 256 features, per-layer block launches for wider ones."""
        if all(a.shape[1] <= 256 and b.shape[1] <= 256 for a, b, _w, _b in jobs):
            ops.wgrad_multi([(a, b, dw, db, None, None) for a, b, dw, db in jobs])
        else:
            for a, b, dw, db in jobs:
                ops.wgrad(a, b, dw, db, n_splits=n_splits)

    # ------------------------------------------------------------------------------------------ training step
    def train_step(self, rgbs, rays, image_indices, n_samples, seg_tokens, perturb=1.0, perturb_rand=None,
                   sigma_noise=None, optimizer_step=True, routing_override=None, grad_allreduce=None, fine_samples=0,
                   fine_u=None, sigma_noise_fine=None, sigma_noise_std=0.0, should_accumulate=None):
        """Runner._training_step + loss assembly + backward + Adam (runner.py:1077-1123, 646-686) = grad_step + apply_step.
        sigma_noise_std: with device noise on (set_device_noise) the std of the sigma noise the step draws itself where none is supplied.
        should_accumulate: with gradient accumulation on (set_accumulation), see apply_step; the result then says whether the optimizer
        stepped (res["optimizer_stepped"]).  The metrics are the micro-batch's own, undivided (the reference's `metrics`)."""
        res = self.grad_step(rgbs, rays, image_indices, n_samples, seg_tokens, perturb, perturb_rand, sigma_noise, routing_override,
                             fine_samples, fine_u, sigma_noise_fine, sigma_noise_std=sigma_noise_std)
        stepped = self.apply_step(grad_allreduce, optimizer_step, should_accumulate=should_accumulate)
        if self.accum_steps > 1:
            res["optimizer_stepped"] = stepped
        return res

    # ------------------------------------------------------------------------------------------ gradient accumulation
    accum_steps = 1                   # A of --accumulation_steps (runner.py:589); 1 = off: no buffer, no extra launch
    accum = None                      # the window's fp32 sum of micro-gradients / A, shaped like self.grad (A > 1 only)
    _micro = 0                        # micro-steps seen since set_accumulation: the reference's train_iterations in its window rule

    def set_accumulation(self, steps: int):
        """Gradient accumulation over `steps` micro-batches (--accumulation_steps, runner.py:589, 657, 677-690): each micro-step's
        gradient is added, divided by `steps`, into self.accum, and the all-reduce, the loss-scale handling, Adam and the refresh of
        the compute copies run on the window's last micro-step only.  Restarts the window (buffer zeroed, micro-step index 0).
        steps = 1 switches accumulation off and frees the buffer."""
        steps = int(steps)
        if steps < 1:
            raise ValueError(f"set_accumulation: accumulation steps must be >= 1, got {steps}")
        if steps > 1 and self.ep is not None and getattr(self.ep, "owner_tail", False):
            raise NotImplementedError(ACCUM_OWNER_TAIL_ERROR)
        self.accum_steps, self._micro = steps, 0
        if steps == 1:
            self.accum = None
        elif self.accum is None:
            self.accum = torch.zeros_like(self.grad)
        else:
            self.accum.zero_()

    def _accumulates(self, should_accumulate=None) -> bool:
        """Whether this micro-step only accumulates - the reference's rule `(train_iterations + 1) % A != 0` (runner.py:589) on the
        model's own micro-step index, or the caller's bool (a run resumed from a checkpoint derives it from its iteration) - and the
        advance of that index."""
        k, self._micro = self._micro, self._micro + 1
        return accumulation_rule(k, self.accum_steps) if should_accumulate is None else bool(should_accumulate)

    def _step_grad(self):
        """The gradient the optimizer step consumes: the flat gradient, or the accumulation buffer while accumulation is on."""
        return self.accum if self.accum_steps > 1 else self.grad

    # ------------------------------------------------------------------------------------------ finite guard
    check_finite = False              # the reference's check_finite (runner.py:620-673; on by default there, off here)
    _guard = None                     # on: dict(ok int32[1], skipped int64[1], step int32[2]) on the device
    _step_host = 0

    @property
    def step_count(self) -> int:
        """Optimizer steps taken (Adam's bias correction).  With the finite guard on the count lives on the device - a step the guard
        drops must not advance it, and nothing in the step reads the flag on the host - and reading it here is a device-to-host read."""
        return int(self._guard["step"][0].item()) if self._guard is not None else self._step_host

    @step_count.setter
    def step_count(self, n: int):
        self._step_host = int(n)
        if self._guard is not None:
            self._guard["step"].copy_(torch.tensor([int(n), 0], dtype=torch.int32))

    def set_check_finite(self, on: bool = True, share=None):
        """The finite guard: a training step whose scalar metrics (photo / gate / total loss, psnr) are not all finite is dropped on
        the device - no Adam step, no step-count advance, gradient accumulation buffer cleared - and counted (skipped_steps()).  A psnr
        of +inf (a perfect reproduction) is allowed.  train_step then returns the device flag as res["step_ok"]; the host reads nothing.
        share: the model whose flag and counter this one uses (the owner of several models - Cascade, BackgroundScene - sets it: one
        check per step covers them all); each model keeps its own device step count.  Off: the step count returns to the host."""
        on = bool(on)
        if on and self.ep is not None and getattr(self.ep, "owner_tail", False):
            raise NotImplementedError(CHECK_FINITE_OWNER_TAIL_ERROR)
        count = self.step_count
        if not on:
            self.check_finite, self._guard = False, None
            self._step_host = count
            return
        i = lambda n, dt: torch.zeros(n, dtype=dt, device=self.dev)
        self._guard = dict(ok=share._guard["ok"] if share is not None else torch.ones(1, dtype=torch.int32, device=self.dev),
                           skipped=share._guard["skipped"] if share is not None else i(1, torch.int64), step=i(2, torch.int32))
        self.check_finite = True
        self.step_count = count
        ops.adam_bias_table(self.dev)          # exists before a capture (read, not created, inside a graph)

    def skipped_steps(self) -> int:
        """Steps the finite guard has dropped so far (a device-to-host read, on demand)."""
        return int(self._guard["skipped"].item()) if self._guard is not None else 0

    def finite_guard_state_dict(self) -> dict:
        """{"check_finite", "skipped_steps", "step_count"} - what a resume needs besides the parameters and Adam's moments; store it
        next to a checkpoint like noise_state_dict (state_dict itself is the reference's parameter key layout and holds tensors only)."""
        return dict(check_finite=self.check_finite, skipped_steps=self.skipped_steps(), step_count=self.step_count)

    def load_finite_guard_state_dict(self, sd: dict):
        self.set_check_finite(bool(sd.get("check_finite", False)))
        self.step_count = int(sd.get("step_count", self.step_count))
        if self._guard is not None:
            self._guard["skipped"].fill_(int(sd.get("skipped_steps", 0)))

    def _finite_guard(self, metrics, psnr_slot: int):
        """The guard's launch behind the loss kernel -> the device flag.  In a torch.distributed run the tail counts the skipped step,
        behind the MIN all-reduce of the flag (optim.apply_tail); otherwise this launch does."""
        g = self._guard
        return ops.finite_guard(metrics, psnr_slot, g["ok"], None if optim.distributed() else g["skipped"])

    def grad_step(self, rgbs, rays, image_indices, n_samples, seg_tokens, perturb=1.0, perturb_rand=None, sigma_noise=None,
                  routing_override=None, fine_samples=0, fine_u=None, sigma_noise_fine=None, split=False, sigma_noise_std=0.0):
        """Forward + loss + backward of one training step: fills self.grad (zeroed first) and returns the metrics.  Nothing here
        depends on host state that changes from step to step, so the whole launch sequence can be captured into a hipGraph
        (graph.GraphedTrainStep).  split=True (plain step only) stops after backward_net_a - the expert block of the gradient is final,
        the launch stream has waited for it - and returns the second half's state as res["bwd_b"] (finish with backward_net_b).
        fine_samples > 0 adds the hierarchical pass (rendering.py:236-268): importance-sample fine depths from the coarse
        weights (detached), evaluate the network on them, sort-merge with the coarse samples, composite the union;
        loss = mse(rgb_fine) + wt * (mean(gate_loss_fine) + mean(gate_loss_coarse)) / 2."""
        N = rays.shape[0]
        self.grad.zero_()
        fine = fine_samples > 0
        if not fine:
            c = out = self.forward_rays(rays, image_indices, n_samples, seg_tokens, perturb, perturb_rand, sigma_noise, True,
                                        routing_override, sigma_noise_std=sigma_noise_std)
        else:
            c, cf, out = self.forward_hier(rays, image_indices, n_samples, fine_samples, seg_tokens, perturb, perturb_rand,
                                           fine_u, sigma_noise, sigma_noise_fine, routing_override, sigma_noise_std=sigma_noise_std)
        # loss (F.mse_loss runner.py:1099, + wt * gate loss :646-651, :1104-1111), psnr and the gradient seeds in ONE launch
        # (swn_step_loss); scaler.scale(loss).backward() (runner.py:679): the scale is read from a DEVICE scalar (kept equal to
        # loss_scaler.scale by _unscale_ok), so a captured step (graph.GraphedTrainStep) follows the scale as it adapts between replays
        ls = self._loss_scale_tensor() if self.loss_scaler is not None else None
        out4, d_rgb, d_la, d_lb = ops.step_loss(out["rgb"], rgbs.to(torch.float32).contiguous(), cf["l_aux"] if fine else c["l_aux"],
                                                c["l_aux"] if fine else None, self.wt, ls)
        photo, gate_loss, loss, psnr = out4[0], out4[1], out4[2], out4[3]
        bwd_b = None
        if split:
            if fine or c.get("parts") is not None or type(self).backward_net is not SwitchNeRF.backward_net:
                raise ValueError("grad_step(split=True): the plain single-context step of a SwitchNeRF only")
            bwd_b = self.backward_net_a(c, ops.composite_bwd(c["raw"], c["z"], d_rgb), d_la, join_side=True)
        elif not fine:
            self.backward(c, d_rgb, d_la)
        else:
            d_raw_m = ops.composite_bwd(out["raw"], out["z"], d_rgb)
            d_raw_f, d_raw_c = ops.unmerge_grad(d_raw_m, out["order"], fine_samples, n_samples)
            self.backward_net(cf, d_raw_f, d_la)
            self.backward_net(c, d_raw_c, d_lb)
        res = dict(loss=loss, photo_loss=photo, gate_loss=gate_loss, psnr=psnr,
                   depth_variance=out["depth_variance"].mean(), ctx=c, rgb=out["rgb"], depth=out["depth"])
        if fine:
            res["ctx_fine"] = cf
        if split:
            res["bwd_b"] = bwd_b
        if self.check_finite:              # (inside a captured step: the flag is device state, like the noise counter)
            res["step_ok"] = self._finite_guard(out4, 3)
        self._noise_advance()              # device noise: the next step draws at step + 1 (the last launch of the captured step)
        return res

    def apply_step(self, grad_allreduce=None, optimizer_step=True, refresh=None, should_accumulate=None, flag_allreduce=None):
        """Gradient all-reduce (N > 1) + Adam (runner.py:486, 686) + refresh of the compute copies of the weights (`refresh`: a
        replacement for refresh_compute_copies, e.g. the replay of its captured graph).
        With gradient accumulation on (set_accumulation(A > 1)) -> whether the optimizer stepped; should_accumulate: None = the
        model's window rule, a bool = the caller's decision for this micro-step (_apply_step_accum)."""
        if self.check_finite:             # the guarded tails are wired in once, in optim.apply_tail: a group of this one model
            stepped = optim.apply_tail([self], grad_allreduce=grad_allreduce, optimizer_step=optimizer_step, refresh=refresh,
                                       should_accumulate=should_accumulate, flag_allreduce=flag_allreduce)
            return stepped if self.accum_steps > 1 else None
        if self.accum_steps > 1:
            return self._apply_step_accum(grad_allreduce, optimizer_step, refresh, should_accumulate)
        if should_accumulate:
            raise ValueError("should_accumulate=True without gradient accumulation: call set_accumulation(steps > 1) first")
        scale = 1.0
        if grad_allreduce is not None:
            scale = grad_allreduce(self._allreduce_view())
        if optimizer_step and self._unscale_ok():
            if self.loss_scaler is not None:
                scale /= self._applied_loss_scale
            self.step_count += 1
            ops.adam_step(self.flat, self.grad, self.m, self.v, None, self.step_count, self.lr, grad_scale=scale)
            (refresh or self.refresh_compute_copies)()

    def _apply_step_accum(self, grad_allreduce, optimizer_step, refresh, should_accumulate) -> bool:
        """apply_step with accumulation on (runner.py:677-690).  An accumulating micro-step adds grad / A into the window's buffer
        and does nothing else: no all-reduce (DDP's no_sync), no inf check, no Adam, no refresh.  The last micro-step without a
        loss scaler and without an all-reduce is ONE launch (swn_adam_accum_step: the last gradient never reaches the buffer, which
        leaves cleared).  Otherwise: add, one all-reduce of the buffer, the inf check on it - the loss scale changes only here, so
        every micro-gradient of a window carried the same scale (GradScaler's accumulation rule) - then Adam from the buffer; a
        skipped step clears the buffer (zero_grad).  optimizer_step=False accumulates like should_accumulate=True."""
        if self.ep is not None and getattr(self.ep, "owner_tail", False):
            raise NotImplementedError(ACCUM_OWNER_TAIL_ERROR)
        inv = 1.0 / self.accum_steps
        if self._accumulates(should_accumulate) or not optimizer_step:
            ops.grad_accum(self.accum, self.grad, inv)
            return False
        if grad_allreduce is None and self.loss_scaler is None:
            self.step_count += 1
            ops.adam_accum_step(self.flat, self.accum, self.grad, self.m, self.v, None, self.step_count, self.lr, accum_scale=inv)
            (refresh or self.refresh_compute_copies)()
            return True
        ops.grad_accum(self.accum, self.grad, inv)
        scale = 1.0
        if grad_allreduce is not None:
            scale = grad_allreduce(self._allreduce_view())
        if not self._unscale_ok():
            self.accum.zero_()
            return False
        if self.loss_scaler is not None:
            scale /= self._applied_loss_scale
        self.step_count += 1
        ops.adam_accum_step(self.flat, self.accum, None, self.m, self.v, None, self.step_count, self.lr, grad_scale=scale)
        (refresh or self.refresh_compute_copies)()
        return True

    _ls_dev = None
    _ls_dev_val = None

    def _loss_scale_tensor(self):
        """The current loss scale as a device scalar (see grad_step), refreshed whenever the host value has changed since the last
        call (after _unscale_ok adapted it, after a checkpoint load, after a caller set loss_scaler.scale)."""
        v = float(self.loss_scaler.scale)
        if self._ls_dev is None:
            self._ls_dev = torch.full((1,), v, dtype=torch.float32, device=self.dev)
        elif self._ls_dev_val != v:
            self._ls_dev.fill_(v)
        self._ls_dev_val = v
        return self._ls_dev

    def _found_inf(self) -> bool:
        """GradScaler's found_inf for THIS model's gradient (one device-to-host flag, like torch's): records the scale the backward
        used (`_applied_loss_scale`, what the Adam step divides by).  Under expert parallelism the expert part of the gradient is
        rank-local (never all-reduced), so the flag is agreed over the ranks (MAX): every rank skips - or takes - the same steps and
        holds the same scale."""
        self._applied_loss_scale = self._ls_dev_val if self._ls_dev_val is not None else self.loss_scaler.scale   # what the backward used
        bad = (~torch.isfinite(self._step_grad()).all()).to(torch.float32).view(1)
        if self.ep is not None and not self.ep.local:
            import torch.distributed as dist
            dist.all_reduce(bad, op=dist.ReduceOp.MAX, group=self.ep.group)
        return bool(bad.item() > 0)

    def _unscale_ok(self) -> bool:
        """GradScaler.step / update (runner.py:686-690): with loss scaling on, skip the optimizer step when a gradient is not finite
        and adapt the scale.  Always True without loss scaling."""
        if self.loss_scaler is None:
            return True
        found_inf = self._found_inf()
        self.loss_scaler.update(found_inf)
        self._loss_scale_tensor()           # the device copy follows (a captured step reads it on its next replay)
        return not found_inf

    def _allreduce_view(self):
        """What the data-parallel all-reduce sums: the whole flat gradient, or - experts sharded over the ranks - its dense
        prefix (a local expert's gradient already holds the contributions of every rank's rows)."""
        g = self._step_grad()           # (the accumulation buffer while accumulation is on: one all-reduce per window)
        if self.ep is not None and not self.ep.local:
            return g[: self.n_dense]
        return g

    def render_forward(self, rays, image_indices, S, F, chunk, perturb, perturb_rand, fine_u, sigma_noise, sigma_noise_fine, *, training,
                       no_batch, routing_override=None, sigma_noise_std=0.0):
        """The render pass of S coarse and F fine samples per ray -> (c, cf, out): forward_hier's result, or for F == 0 the one context
        of forward_rays as (c, None, c).  The forward of the autograd bridge, of the captured render graphs and of the eager render_rays
        (grad_step writes the same two calls out itself); the caller advances the noise counter (_noise_advance) where its step ends."""
        if F > 0:
            return self.forward_hier(rays, image_indices, S, F, chunk, perturb, perturb_rand, fine_u, sigma_noise, sigma_noise_fine,
                                     routing_override, no_batch, training, sigma_noise_std)
        c = self.forward_rays(rays, image_indices, S, chunk, perturb, perturb_rand, sigma_noise, training, routing_override,
                              no_batch=no_batch, sigma_noise_std=sigma_noise_std)
        return c, None, c

    def render_backward(self, c, cf, out, d_rgb, d_laux_c, d_laux_f):
        """Backward of render_forward given dL/d rgb [N,3] and each level's dL/d l_aux[seg]: accumulates into self.grad, the fine level
        first."""
        if cf is None:
            return self.backward(c, d_rgb, d_laux_c)
        d_raw_f, d_raw_c = hier.merged_bwd(out, d_rgb)
        self.backward_net(cf, d_raw_f, d_laux_f)
        self.backward_net(c, d_raw_c, d_laux_c)

    def hier_passes(self, rays, image_indices, n_samples, fine_samples, seg_tokens, perturb, perturb_rand, fine_u, sigma_noise,
                    sigma_noise_fine, routing_override, no_batch, training, sigma_noise_std):
        """forward_hier up to the compositing of the union: coarse pass (composited for its weights, its raw outputs kept), importance
        sampling of the fine depths from the detached coarse weights, fine pass on those depths, sort-merge of both sample sets
        (rendering.py:419-433) -> (coarse ctx, fine ctx, z_fine, merged z, order, merged raw).  BackgroundScene.forward composites the
        union with its own bounded kernel."""
        N = rays.shape[0]
        c = self.forward_rays(rays, image_indices, n_samples, seg_tokens, perturb, perturb_rand, sigma_noise, training,
                              routing_override, no_batch=no_batch, want_weights=True, sigma_noise_std=sigma_noise_std)
        if fine_u is None and perturb != 0 and training and self.noise.on:      # device noise: stream 2
            fine_u = self.noise.draw(ops.RNG_FINE_U, N * fine_samples, self.noise.base * fine_samples,
                                     ops.RNG_UNIFORM).view(N, fine_samples)
        if fine_u is None:
            fine_u = hier.default_fine_u(self._linspace, N, fine_samples, perturb, self.dev)
        z_fine = ops.sample_pdf(c["z"], c["weights"], fine_u, fine_samples)
        seg_f = min(seg_tokens, N * fine_samples)
        cf = self.forward_rays(rays, image_indices, fine_samples, seg_f, 0.0, None, sigma_noise_fine, training, None,
                               no_batch=no_batch, z_in=z_fine, pe_dir=c["pe_dir"], tag="f", composite=False,
                               sigma_noise_std=sigma_noise_std)
        zm, order, raw_m = ops.merge_samples(z_fine, c["z"], cf["raw"], c["raw"])
        return c, cf, z_fine, zm, order, raw_m

    def forward_hier(self, rays, image_indices, n_samples, fine_samples, seg_tokens, perturb=0.0, perturb_rand=None,
                     fine_u=None, sigma_noise=None, sigma_noise_fine=None, routing_override=None, no_batch=False, training=True,
                     sigma_noise_std=0.0):
        """_get_results with fine_samples > 0 and no cascade (rendering.py:199-274): hier_passes and the compositing of the union.
        Returns (coarse ctx, fine ctx, merged results {raw, z, order, z_fine, rgb, depth, depth_variance})."""
        c, cf, z_fine, zm, order, raw_m = self.hier_passes(rays, image_indices, n_samples, fine_samples, seg_tokens, perturb, perturb_rand,
                                                           fine_u, sigma_noise, sigma_noise_fine, routing_override, no_batch, training,
                                                           sigma_noise_std)
        out = dict(raw=raw_m, z=zm, order=order, z_fine=z_fine)
        out["rgb"], out["depth"], out["depth_variance"], _ = ops.composite_fwd(raw_m, zm)
        return c, cf, out

    # ------------------------------------------------------------------------------------------ mip path
    def forward_level_mip(self, rays, radii, image_indices, z, seg_tokens, sigma_noise=None, no_batch=False, tag="c",
                          want_weights=False, rgb_padding=0.001, pe_dir=None, training=True, sigma_noise_std=0.0):
        """One level of rendering_mip._get_results (rendering_mip.py:195-215 / :236-253): the S edges `z` of every ray give
        S - 1 conical frustums; integrated positional encoding (swn_mip_encode) -> the same network (MipNeRFMoE.forward is
        NeRFMoE.forward behind MipEmbedder, nerf_moe.py:675-810) -> compositing at the frustum mid points with the colour
        padding of :383-386."""
        N, S1 = rays.shape[0], z.shape[1] - 1
        self._sync_compute_copies()
        pe = ops.mip_encode(rays, radii, z, self.cfg["pos_xyz_dim"], self.dtype, self.KP)
        if pe_dir is None:
            pe_dir = self._dir_pe(rays)
        seg = min(seg_tokens, N * S1)
        drawn = None
        if training and self.noise.on and sigma_noise is None and sigma_noise_std > 0:      # one value per interval
            sigma_noise = drawn = self.noise.draw(ops.RNG_SIGMA if tag == "c" else ops.RNG_SIGMA_FINE, N * S1, self.noise.base * S1,
                                                  ops.RNG_NORMAL, float(sigma_noise_std))
        c = self._net_forward(pe, pe_dir, image_indices, N, S1, seg, sigma_noise, None, no_batch, tag, saving=bool(training))
        c["z_edges"] = z
        if drawn is not None:
            c["sigma_noise"] = drawn
        c["z"] = (0.5 * (z[:, 1:] + z[:, :-1])).contiguous()
        c["rgb_padding"] = float(rgb_padding)
        c["rgb"], c["depth"], c["depth_variance"], c["weights"] = ops.composite_fwd(c["raw"], c["z"], want_weights=want_weights,
                                                                                    rgb_padding=rgb_padding)
        return c

    def forward_mip(self, rays, radii, image_indices, n_samples, n_fine, seg_tokens, perturb=0.0, perturb_rand=None, fine_u=None,
                    sigma_noise=None, sigma_noise_fine=None, no_batch=False, rgb_padding=0.001, resample_padding=0.01,
                    training=True, fine_randomized=None, sigma_noise_std=0.0):
        """rendering_mip.render_rays (rendering_mip.py:133-172): coarse level on n_samples edges, then (n_fine > 0) the fine
        level on n_fine edges resampled from the blurred coarse weights (stop_level_grad: no gradient through the edges).
        fine_u: the U[0,1) tensor [N, n_fine] of sorted_piecewise_constant_pdf1's randomized branch (drawn here if perturb > 0
        and none is given); perturb = 0 -> deterministic.  fine_randomized (default: perturb > 0) decouples the fine level's
        randomisation from the coarse jitter: the reference resamples with randomized=hparams.perturb even in eval mode
        (rendering_mip.py:227) while its coarse jitter is off there (:147).  training=False skips the activation saves."""
        N = rays.shape[0]
        if fine_randomized is None:
            fine_randomized = perturb > 0
        t_steps = self._linspace(n_samples)
        radii = radii.reshape(-1).contiguous()
        dn = self.noise if training and self.noise.on else None
        if dn is not None and perturb > 0 and perturb_rand is None:       # device noise: stream 0 through the fill
            perturb_rand = dn.draw(ops.RNG_JITTER, N * n_samples, dn.base * n_samples, ops.RNG_UNIFORM).view(N, n_samples)
        z = ops.sample_z(rays, t_steps, perturb_rand, perturb, n_samples)
        c = self.forward_level_mip(rays, radii, image_indices, z, seg_tokens, sigma_noise, no_batch, "c", n_fine > 0, rgb_padding,
                                   training=training, sigma_noise_std=sigma_noise_std)
        if n_fine <= 0:
            return c, None
        if fine_u is None and fine_randomized and dn is not None:          # stream 2
            fine_u = dn.draw(ops.RNG_FINE_U, N * n_fine, dn.base * n_fine, ops.RNG_UNIFORM).view(N, n_fine)
        if fine_u is None and fine_randomized:
            fine_u = torch.rand(N, n_fine, device=self.dev)
        z_f = ops.mip_resample(z, c["weights"], fine_u if fine_randomized else None, n_fine, resample_padding)
        cf = self.forward_level_mip(rays, radii, image_indices, z_f, seg_tokens, sigma_noise_fine, no_batch, "f", False, rgb_padding,
                                    pe_dir=c["pe_dir"], training=training, sigma_noise_std=sigma_noise_std)
        return c, cf

    def train_step_mip(self, rgbs, rays, radii, image_indices, n_samples, n_fine, seg_tokens, perturb=1.0, perturb_rand=None,
                       fine_u=None, sigma_noise=None, sigma_noise_fine=None, optimizer_step=True, grad_allreduce=None,
                       rgb_padding=0.001, resample_padding=0.01, sigma_noise_std=0.0):
        """Runner._training_step_mip (runner.py:1126-1167): loss = (mse(rgb_fine) + mse(rgb_coarse)) / 2
        + wt * (mean(gate_loss_fine) + mean(gate_loss_coarse)) / 2, backward through both levels, Adam."""
        if self.accum_steps > 1:
            raise NotImplementedError("train_step_mip: gradient accumulation (set_accumulation) is not built for the mip step")
        if self.check_finite:
            raise NotImplementedError("train_step_mip: the finite guard (check_finite) is not built for the mip step")
        self.grad.zero_()
        c, cf = self.forward_mip(rays, radii, image_indices, n_samples, n_fine, seg_tokens, perturb, perturb_rand, fine_u,
                                 sigma_noise, sigma_noise_fine, False, rgb_padding, resample_padding, sigma_noise_std=sigma_noise_std)
        levels = [c] if cf is None else [cf, c]
        share = 1.0 / len(levels)
        photo, gate_loss = 0.0, 0.0
        ls = self._loss_scale_tensor() if self.loss_scaler is not None else 1.0
        for lv in levels:
            diff = lv["rgb"] - rgbs
            lv["_d_rgb"] = (diff * (2.0 * share / diff.numel()) * ls).contiguous()
            photo = photo + share * (diff * diff).mean()
            gate_loss = gate_loss + share * lv["l_aux"].mean()
        loss = photo + self.wt * gate_loss
        for lv in levels:
            d_raw = ops.composite_bwd(lv["raw"], lv["z"], lv["_d_rgb"], rgb_padding=lv["rgb_padding"])
            d_laux = torch.full((lv["n_seg"],), share * self.wt / lv["n_seg"], dtype=torch.float32, device=self.dev) * ls
            self.backward_net(lv, d_raw, d_laux)
        self._noise_advance()
        self.apply_step(grad_allreduce, optimizer_step)
        top = levels[0]
        return dict(loss=loss, photo_loss=photo, gate_loss=gate_loss, psnr=-10.0 * torch.log10(((top["rgb"] - rgbs) ** 2).mean()),
                    depth_variance=top["depth_variance"].mean(), ctx=c, ctx_fine=cf, rgb=top["rgb"], depth=top["depth"])

    def set_iteration(self, iteration: int, lr_decay_factor: float = 0.1, train_iterations: int = 500000):
        """Learning-rate schedule hook = the reference's ExponentialLR(gamma = lr_decay_factor ** (1 / train_iterations)) stepped
        once per iteration (runner.py:505-512, 688-693): the rate the step of `iteration` (0-based) uses."""
        from . import checkpoint
        self.lr = checkpoint.exponential_lr(self.base_lr, iteration, lr_decay_factor, train_iterations)
        return self.lr

    # ------------------------------------------------------------------------------------------ NeRFMoE mirrors
    training = True
    moe_no_batch = False

    def train(self, mode=True):
        self.training = bool(mode)
        return self

    def eval(self):
        return self.train(False)

    def modules(self):
        """nn.Module.modules() stand-in: Runner.set_no_batch (runner.py:946-951) walks it looking for `moe_no_batch`."""
        yield self

    def named_parameters(self):
        """(reference key, tensor) pairs - the parameters in the reference's key layout, for inspection / count_parameters
        (runner.py:196-199).  The trainable leaf an optimizer should be given is `flat_param` (trainable_parameters())."""
        return iter(self._to_ref_layout(self.p).items())

    def parameters(self):
        return (v for _, v in self.named_parameters())

    # ---- torch.autograd bridge (autograd.py): the reference's Runner loop drives the HIP path unchanged
    _flat_param = None
    _packed_version = -1

    @property
    def flat_param(self):
        """The model's whole parameter set as ONE leaf nn.Parameter sharing storage with the flat fp32 master buffer.  Give it to
        torch.optim.Adam / DDP; rendering.render_rays(...) in training mode returns tensors whose backward fills its `.grad`."""
        if self._flat_param is None:
            self._flat_param = torch.nn.Parameter(self.flat, requires_grad=True)
            self._packed_version = self._flat_param._version
        return self._flat_param

    def trainable_parameters(self):
        return [self.flat_param]

    def _sync_compute_copies(self):
        """An optimizer outside this class moved the master weights in place (the Parameter's version counter tells): refresh the
        packed compute copies the chain kernels read."""
        fp = self._flat_param
        if fp is not None and fp._version != self._packed_version:
            self.refresh_compute_copies()
            self._packed_version = fp._version

    def to(self, *_a, **_k):
        return self

    def set_no_batch(self, mode=True):
        """NeRFMoE.set_no_batch (models/nerf_moe.py:315-318): eval path without capacity / token dropping."""
        self.moe_no_batch = bool(mode)

    def __call__(self, x, sigma_only=False, sigma_noise=None):
        """NeRFMoE.forward (models/nerf_moe.py:320-455): x [P, 7] = xyz(3), dir(3), image index(1) ->
        {"outputs": [P,4] (rgb, sigma), "extras": {"moe_loss": [1], "moe_gates": [[P,1]]}}.  Routing (capacity, ranking,
        l_aux) is over the P points of this call, exactly like one model chunk of the reference.  Inference only."""
        expected = 7
        if x.shape[1] != expected:
            raise Exception("Unexpected input shape: {} (expected: {}, xyz_dim: {})".format(x.shape, expected, 3))
        P = x.shape[0]
        xf = x.to(torch.float32)
        rays = torch.cat([xf[:, :6], torch.zeros(P, 2, device=self.dev)], 1).contiguous()   # o = xyz, z = 0 -> sample = xyz
        c = self.forward_rays(rays, xf[:, 6].long().contiguous(), 1, P, 0.0, None,
                              None if sigma_noise is None else sigma_noise.reshape(-1).to(torch.float32).contiguous(),
                              training=self.training, no_batch=self.moe_no_batch)
        return {"outputs": c["raw"], "extras": {"moe_loss": c["l_aux"], "moe_gates": [c["idx"].long().view(P, 1)]}}
