"""Family-neutral part of the vision-tower step engines (`TowerEngine`): the flat parameter store and its views, the trainable /
decay flags, the fold guard of the frozen schedule, and the tower-level drivers -- encode_image (teacher), encode_dense / backward_dense
(student), RoI pooling, AdamW.  Nothing here names a parameter of one tower family: layout, stem, blocks and head belong to the
subclasses (engine.py: EVA02, engine_openai.py: OpenAI-CLIP ViT), which plug into the drivers through the few hooks listed on the class.
"""
from __future__ import annotations

import math
import os
from collections import OrderedDict

import torch
import torch.nn.functional as F

from .config import TowerCfg

BF16, F32 = torch.bfloat16, torch.float32
EPI_BF16, EPI_F32, EPI_RESID_F32, EPI_SWIGLU_BF16, EPI_ATOMIC_F32, EPI_PATCH_F32, EPI_RESID_LN_F32, EPI_GELU_BF16, EPI_QGELU_BF16 = range(9)
DX_BF16, DX_F32_ASSIGN, DX_F32_ACCUM = range(3)
ALIGN = 64


def _round_up(x: int, m: int) -> int:
    return (x + m - 1) // m * m


def padded_hidden(cfg: TowerCfg) -> int:
    return _round_up(cfg.hidden, 64)


def is_no_decay(name: str, ndim: int) -> bool:
    """AdamW grouping rule of the reference (src/training/main.py:199)."""
    return ndim < 2 or "bn" in name or "ln" in name or "bias" in name or "logit_scale" in name


class TowerEngine:
    """A family supplies, besides its layout (`_layout`), stem (`_stem`, `_stem_bwd`), blocks (`_block_fwd`, `_teacher_block_folded`,
    `_block_bwd`), `rope_tables`, `sync_transposed` and `_build_folds`, the hooks below.  What both families schedule alike is written once
    here on those hooks: the CLS-only last block (`_block_fwd_cls`), the q|k|v GEMM and the residual GEMMs of `_teacher_block_folded`
    (`_teacher_qkv`, `_resid_gemm_folded`), the head of the backward pass (`_bwd_workspaces`, `_final_norm_bwd`) and the W^T shadows of
    the trainable blocks (`_block_wt_pairs`).
      names    BLOCK_TAG, NORM1, FINAL_NORM, RESID_BIAS, _pos_table(views)
      blocks   _qkv_operands (the stacked q|k|v matrix and bias), _block_tail (the block behind the attention core, for whichever rows
               it is given), _block_linears (the four linears of a block: key, bf16 matrix)
      head     _head (forward), _head_dgrad, _head_wgrad (the train-all weight / bias gradients)
      teacher  _fold_pass (does this pass fold?), _cls_block_folds, _lo_plane (is the low plane of the split stream allocated?)
      student  _bwd_widths (LayerNorm / column-sum workspace widths), _bwd_gq
      shadows  HEAD_FWD_TRANSPOSED, _wants_folds (what sync_shadow rebuilds for a frozen tower)"""
    BLOCK_TAG = None                          # state-dict name of the block list below the tower prefix
    NORM1 = None                              # ... of a block's first LayerNorm below the block's prefix
    FINAL_NORM = None                         # ... of the final LayerNorm
    RESID_BIAS = None                         # tail of a block's second residual bias: its gradient comes out of the LayerNorm backwards
    HEAD_FWD_TRANSPOSED = False               # does the forward head GEMM read a transposed shadow (then frozen towers need sync_transposed too)

    def block_index(self, name: str):
        """Index of the transformer block a state-dict name belongs to, None for stem / head tensors."""
        tag = self.prefix + self.BLOCK_TAG
        return int(name[len(tag):].split(".")[0]) if name.startswith(tag) else None

    def _b(self, i: int) -> str:
        """State-dict name prefix of block i."""
        return f"{self.prefix}{self.BLOCK_TAG}{i}."

    def _never_reached(self, i: int, name: str) -> bool:
        """Tensors of block i the dense path never differentiates (none, unless a family says otherwise)."""
        return False

    def __init__(self, cfg: TowerCfg, ops, trainable: bool = False, prefix: str = "visual."):
        self.cfg, self.ops, self.prefix, self.trainable = cfg, ops, prefix, trainable
        self.offsets = OrderedDict()          # name -> (offset, storage shape)
        self.logical = {}                     # name -> logical (reference) shape
        off = 0
        self.block_ranges = []                # flat [begin, end) of each block (contiguous all-reduce buckets)
        cur_block, blk_begin = None, 0
        for grp in self._layout():
            off = _round_up(off, ALIGN)
            blk = self.block_index(grp[0][0])
            if blk != cur_block:
                if cur_block is not None:
                    self.block_ranges.append((blk_begin, off))
                cur_block, blk_begin = blk, off
            for name, shape, storage in grp:
                self.offsets[name] = (off, storage)
                self.logical[name] = shape
                off += math.prod(storage)
        self.numel = _round_up(off, 256)
        # stem (class token, position embedding, patch embedding) and head (final norm, head) slices of the flat store: two more gradient
        # buckets when the whole tower trains (training without --lock-image)
        self.stem_range = (0, self.block_ranges[0][0]) if self.block_ranges else (0, 0)
        self.head_range = (self.block_ranges[-1][1], self.numel) if self.block_ranges else (0, self.numel)
        self.master = ops.zeros((self.numel,), F32)
        self.shadow = ops.zeros((self.numel,), BF16)
        self.device = self.master.device
        self.Hp = padded_hidden(cfg)
        self.Kpe = _round_up(3 * cfg.patch_size * cfg.patch_size, 64)
        self.p = {n: self.view_of(self.master, n) for n in self.offsets}
        self.w = {n: self.view_of(self.shadow, n) for n in self.offsets}
        self._tables = {}
        self._pos_cache = {}
        self.grad = self.exp_avg = self.exp_avg_sq = self.flags = None
        self.guard = None                      # cs_adamw_step's guard buffer (norm, clip coefficient, applied, skipped steps): first guarded adamw_step
        self.g = {}
        self.wt = {}
        self.first_trainable = cfg.layers      # no block trainable until lock()/unlock is applied
        self.train_all = False                 # stem + final norm + head train as well (set_trainable_all: training without --lock-image)
        self.flags_version = 0                 # bumped whenever the trainable / decay flag bytes are rewritten (_set_flags)
        self.grad_ready_hook = None            # callable(block_index) fired when a block's grads are complete
        self._ctx = None
        self._wgrad_ws = None
        # encode_image() consumes only the CLS row, so the last block runs its query/proj/MLP for that row alone (keys and
        # values still span all tokens); False runs the last block over every token -- same outputs, ~1/L more work.
        self.cls_only_last_block = True
        # Frozen towers, encode_image(): the two block LayerNorms are applied inside the GEMMs that consume them -- gamma goes into a bf16
        # copy of the weight, beta and the row statistics into the GEMM epilogue; the residual GEMMs also emit a bf16 copy of the new
        # stream and its row statistics (_teacher_block_folded)
        self.fold_block_ln = not trainable
        # Guard of that fold.  The folded LayerNorms contract the UN-centred bf16 row and remove the mean afterwards in fp32
        # (rstd * (bf16(x) . W gamma - mean * colsum)): the bf16 rounding of x is relative to |x|, not to |x - mean|, so the error of the
        # normalised row grows like sqrt(1 + (mean / sigma)^2).  Measured against the plain schedule on weights with trained-like statistics
        # (oracle/stress_weights.py, profiles/r04_parity.md): outlier channels x200 alone -- folded is CLOSER to fp32 than the plain bf16
        # schedule; |mean| / sigma = 2 -- equal; 3 -- 1.6x; 5 -- 2.8x (whole tower: the frozen schedule's saved roundings elsewhere offset the
        # fold's cost up to 2).  One LayerNorm -> GEMM alone, against fp64 (profiles/ln_conditioning.md, tests/test_gpu_ln_cond.py): folded /
        # plain = 0.99 at 0, 1.13 at 1, 1.49 at 2, 1.91 at 3, 2.86 at 5 -- error^2 = floor^2 + b^2 (1 + r^2), the law diluted by the
        # roundings both chains share; the limit of 2 thus caps a single fold at 1.5x.  So the first encode_image() after a weight load measures
        # mean_rows(|row mean| / row sigma) of the stream entering every block on a few crops (block_fold_statistic, one host read-back)
        # and keeps the block LayerNorms as LayerNorm kernels when it exceeds block_fold_limit.
        self.block_fold_guard = not trainable
        self.block_fold_limit = 2.0
        self.block_fold_ratio = None           # the measured statistic (None: not measured since the last weight load)
        # ... with the residual stream between those GEMMs held as two 16-bit planes (bf16 view + remainder, exact; cs_gemm_nt_ln_split):
        # 8 instead of 10 bytes of HBM traffic per stream element and residual GEMM
        self.split_stream = not trainable
        self.fold = {}
        # (leading blocks, CUs): encode_image()'s persistent GEMMs leave that many compute units free in its first blocks -- set by
        # CLIPSelf.prefetch_teacher in data-parallel runs, where those blocks run beside the student's gradient all-reduce
        self.rccl_window = (0, 0)
        self.wgrad_tn = True                   # weight gradients from the token-major operands (no transposed copies) where the shape allows
        if trainable:
            self.grad = ops.zeros((self.numel,), F32)
            self.exp_avg = ops.zeros((self.numel,), F32)
            self.exp_avg_sq = ops.zeros((self.numel,), F32)
            self.g = {n: self.view_of(self.grad, n) for n in self.offsets}
            self.flags = torch.zeros(self.numel // 64, dtype=torch.uint8, device=self.device)

    # ------------------------------------------------------------------------------------------ parameters
    def storage_of(self, buf, name):
        """The (possibly zero-padded) storage block of `name` inside a flat buffer, in its storage shape."""
        o, st = self.offsets[name]
        return buf[o:o + math.prod(st)].view(st)

    def view_of(self, buf, name):
        """The reference-shaped tensor of `name` inside a flat buffer: a plain view, or a strided view of the leading
        block when the storage is padded."""
        o, st = self.offsets[name]
        shape = self.logical[name]
        flat = buf[o:o + math.prod(st)]
        if tuple(st) == tuple(shape) or math.prod(st) == math.prod(shape):
            return flat.view(shape)
        if len(st) == 1:
            return flat[:shape[0]]
        if len(shape) == 2:
            return flat.view(st)[:shape[0], :shape[1]]
        inner = [1]
        for d in reversed(shape[2:]):
            inner.insert(0, inner[0] * d)                 # contiguous strides of the trailing dims
        return torch.as_strided(flat, shape, (st[1], *inner))

    def public_names(self):
        return [n for n in self.offsets if "._" not in n]

    def load_state(self, sd: dict, strict: bool = True):
        missing = []
        with torch.no_grad():
            for n in self.public_names():
                if n in sd:
                    self.p[n].copy_(sd[n].to(self.device, F32).reshape(self.p[n].shape))
                else:
                    missing.append(n)
        if strict and missing:
            raise KeyError(f"missing keys: {missing[:5]}... ({len(missing)})")
        self.sync_shadow()
        return missing

    def sync_shadow(self):
        """bf16 MFMA operands from the fp32 masters (after a load; AdamW refreshes them itself each step), and what is derived from them."""
        self.ops.cast_f32_bf16(self.master, self.shadow)
        self._pos_cache.clear()
        self.block_fold_ratio = None
        if self.trainable or self.HEAD_FWD_TRANSPOSED:
            self.sync_transposed()
        if self._wants_folds():
            self._build_folds()

    def _wants_folds(self) -> bool:
        return self.fold_block_ln

    def _wt_alloc(self, key, rows, cols):
        t = self.wt.get(key)
        if t is None:
            t = self.ops.zeros((cols, _round_up(rows, 64)), BF16)
            self.wt[key] = t
        return t

    def _block_wt_pairs(self, blocks=None):
        """(W, its W^T shadow) for every linear of the trainable blocks (or of `blocks`), in block order: the dgrad operands' part of the
        list a family's sync_transposed hands to the one batched transpose."""
        blocks = range(self.first_trainable, self.cfg.layers) if blocks is None else blocks
        return [(W, self._wt_alloc((i, key), *W.shape)) for i in blocks for key, W in self._block_linears(i)]

    def set_trainable_blocks(self, unlocked_groups: int):
        """visual.lock(unlocked_groups) (eva_vit_model.py:500-516): only the last n blocks train
        (blocks[-0:] is the whole list, as in the reference).  A family whose lock() knows more groups than blocks extends this."""
        L = self.cfg.layers
        self.first_trainable = L - unlocked_groups if 0 < unlocked_groups <= L else 0
        self.train_all = False
        self._set_flags()

    def set_trainable_all(self):
        """No lock at all (training.main without --lock-image, src/training/main.py:161-166): every parameter of the visual tower trains --
        besides the blocks the stem (class token, position table, patch embedding), the final norm and the head, which the dense path
        differentiates as well."""
        self.first_trainable = 0
        self.train_all = True
        self._set_flags()

    def _set_flags(self):
        if not self.trainable:
            return
        self.flags.zero_()
        names = list(self.offsets)
        for k, name in enumerate(names):
            o, s = self.offsets[name]
            i = self.block_index(name)
            if "._" in name or (i is None and not self._nonblock_trains(name)) or (i is not None and (i < self.first_trainable or self._never_reached(i, name))):
                continue
            n = math.prod(s)
            nxt = self.offsets[names[k + 1]][0] if k + 1 < len(names) else self.numel
            n64 = _round_up(n, 64)            # a tensor that ends its 64-aligned allocation group short of a flag granule (tiny head.bias)
            assert o % 64 == 0 and (n % 64 == 0 or o + n64 <= nxt), f"{name}: flag granularity"
            self.flags[o // 64:(o + n64) // 64] = 1 | (0 if is_no_decay(name, len(self.logical[name])) else 2)
        self.flags_version += 1
        # W^T shadows that only trainable blocks need: drop those of blocks that are frozen now, build the missing ones of blocks that train now
        for key in [k for k in self.wt if isinstance(k, tuple) and k[0] < self.first_trainable]:
            del self.wt[key]
        self.sync_transposed()

    def _nonblock_trains(self, name):
        """Does a tensor outside the blocks (stem, final norm, head) train?  By default only without --lock-image (set_trainable_all)."""
        return self.train_all

    def _pos_trains(self):
        """Does the position table train?  It is the first stem tensor to unlock in every family, so this also says whether the stem
        backward runs (encode_dense keeps the stem activations for it) and whether AdamW invalidates the rescaled tables."""
        return self.train_all

    def trainable_names(self):
        if self.train_all:
            return self.public_names()
        return [n for n in self.public_names()
                if (self.block_index(n) >= self.first_trainable if self.block_index(n) is not None else self._nonblock_trains(n))]

    def bucket_range(self, key):
        """Flat [begin, end) of a gradient bucket: a block index, "head" (final norm + head) or "stem" (cls_token, pos_embed, patch embedding)."""
        return self.head_range if key == "head" else self.stem_range if key == "stem" else self.block_ranges[key]

    # ------------------------------------------------------------------------------------------ position embedding
    def pos_for(self, grid: int):
        """Position table [N, C] fp32, bicubic-rescaled for a non-native grid (eva_vit_model.py:631-643, transformer.py:724-734).  One-time
        host-side table preparation per grid size, cached."""
        if grid not in self._pos_cache:
            pe = self._pos_table(self.p)
            if grid != self.cfg.grid:
                C = pe.shape[1]
                pe2 = pe[1:].T.contiguous().view(1, C, self.cfg.grid, self.cfg.grid)
                pe2 = F.interpolate(pe2, (grid, grid), mode="bicubic", align_corners=False).view(C, grid * grid)
                pe = torch.cat([pe[:1], pe2.T], dim=0)
            self._pos_cache[grid] = pe.contiguous()
        return self._pos_cache[grid]

    def _pos_grad(self, d_pos, grid):
        """Position-table gradient += d_pos [N, C] (already summed over images), through the bicubic rescale for a non-native grid."""
        cfg, C = self.cfg, self.cfg.width
        gpos = self._pos_table(self.g)                                          # [native N, C]
        if grid == cfg.grid:
            gpos.add_(d_pos)
            return
        gpos[0].add_(d_pos[0])
        with torch.enable_grad():
            pe = self._pos_table(self.p).detach()[1:].T.reshape(1, C, cfg.grid, cfg.grid).clone().requires_grad_(True)
            out = F.interpolate(pe, (grid, grid), mode="bicubic", align_corners=False)
            (d_pe,) = torch.autograd.grad(out, pe, d_pos[1:].T.reshape(1, C, grid, grid))
        gpos[1:].add_(d_pe.reshape(C, cfg.grid * cfg.grid).T)

    @staticmethod
    def _join_planes(hi, lo):
        """fp32 values of a split stream (cs_gemm_nt_ln_split: hi | lo = the halves of bits(x) + 0x8000); used on the B CLS rows only."""
        y = (hi.contiguous().view(torch.int16).to(torch.int32) << 16) | (lo.to(torch.int32) & 0xFFFF)
        return (y - 0x8000).view(torch.float32)

    # ------------------------------------------------------------------------------------------ teacher
    def fold_probe(self, crops: int = 16, kind: str = "white"):
        """The crops the guard is calibrated on, seeded (numpy PCG64, version-stable) at the tower's native size -- the same on every rank, in
        every run and whatever the first batch holds, so that all ranks of a data-parallel job choose the same teacher schedule and two runs of
        one checkpoint produce the same distillation targets.  (The statistic is a property of the weights -- massive-activation channels,
        bias-driven row means -- far more than of the pixels; oracle/stress_weights.py builds it from them.)  Two kinds (white
        noise alone can under-estimate a common-mode row mean that real crops excite): "white" = N(0, 1) pixels; "natural" = what
        normalised photographs look like to a patch embedding -- a 1/f amplitude spectrum (smooth regions, few edges) around a per-image,
        per-channel mean of N(0, 1), i.e. crops that are mostly one colour.  The guard takes the larger statistic of the two."""
        import numpy as np
        S = self.cfg.image_size
        g = np.random.Generator(np.random.PCG64(20250927 if kind == "white" else 20251001))
        x = g.standard_normal((crops, 3, S, S), dtype=np.float32)
        if kind == "natural":
            f = np.hypot(np.fft.fftfreq(S)[:, None], np.fft.rfftfreq(S)[None, :]).astype(np.float32)
            f[0, 0] = 1.0
            x = np.fft.irfft2(np.fft.rfft2(x) / f, s=(S, S)).astype(np.float32)
            x -= x.mean(axis=(2, 3), keepdims=True)
            x /= x.std(axis=(2, 3), keepdims=True) + 1e-6
            x = 0.5 * x + g.standard_normal((crops, 3, 1, 1), dtype=np.float32)
        elif kind != "white":
            raise ValueError(kind)
        return torch.from_numpy(np.ascontiguousarray(x)).to(self.device)

    def block_fold_statistic(self, images=None, crops: int = 16):
        """max over blocks of mean over rows of |row mean| / row sigma of the residual stream entering the block, on `images[:crops]`
        (default: the larger of the two fold_probe() kinds) through the plain block schedule.  One-time calibration after a weight load (a
        few torch reductions and one host read-back per probe, not part of the step)."""
        if images is None:
            return max(self.block_fold_statistic(self.fold_probe(crops, kind), crops) for kind in ("white", "natural"))
        with torch.no_grad():
            img = images[:crops]
            B = img.shape[0]
            x, g = self._stem(img)
            N = g * g + 1
            cos, sin = self.rope_tables(g)
            xf = x.view(B * N, self.cfg.width)
            worst = xf.new_zeros(())
            for i in range(self.cfg.layers):
                worst = torch.maximum(worst, (xf.mean(-1).abs() / xf.std(-1).clamp_min(1e-30)).mean())
                if i + 1 < self.cfg.layers:
                    self._block_fwd(i, xf, B, N, cos, sin, True, None, True)
            return float(worst)

    @staticmethod
    def _fold_group_active() -> bool:
        import torch.distributed as dist
        # (CLIPSELF_FORCE_DIST=1: the one-rank rehearsal of the N-rank path takes the collective too -- the only way to run this RCCL call on a one-GPU box)
        return dist.is_available() and dist.is_initialized() and (dist.get_world_size() > 1 or os.environ.get("CLIPSELF_FORCE_DIST") == "1")

    def calibrate_block_folds(self, collective: bool = True) -> bool:
        """Measure the guard's statistic of the current weights on the seeded probes and decide whether norm1 / norm2 are folded.  In a process
        group (collective=True) every rank takes the MAX over ranks -- one scalar all-reduce --, so the ranks cannot disagree even if their
        devices rounded differently.  That makes this a COLLECTIVE call: every rank must reach it at the same point of the program --
        training.main does right after a frozen tower's weights are in place (FrozenDataParallel.__init__, and after the evaluation model's
        load_state_dict), never from inside a forward pass that some rank might skip (an empty evaluation shard used to hang the
        job there).  An error of the collective is an error of the job and propagates.  The statistic and the decision are logged once per
        calibration."""
        import logging
        ratio = self.block_fold_statistic()
        agreed = ""
        if collective and self._fold_group_active():
            import torch.distributed as dist
            t = torch.tensor([ratio], dtype=torch.float64, device=self.device if dist.get_backend() == "nccl" else "cpu")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            ratio = float(t[0])
            agreed = f", MAX over {dist.get_world_size()} ranks"
        self.block_fold_ratio = ratio
        folded = ratio <= self.block_fold_limit
        near = abs(ratio - self.block_fold_limit) <= 0.1 * self.block_fold_limit
        logging.log(logging.WARNING if (near or not folded) else logging.INFO,
                    "frozen tower: mean |row mean| / row sigma of the residual stream = %.3f on the seeded probes%s (limit %.1f%s) -- norm1 / norm2 %s",
                    ratio, agreed, self.block_fold_limit, ", within 10 % of it" if near else "",
                    "folded into the q|k|v and W1|W2 GEMMs" if folded else
                    "stay LayerNorm kernels (the folded form would lose precision on these weights)")
        return folded

    def block_folds_active(self, images=None) -> bool:
        """Whether encode_image() folds norm1 / norm2 into the q|k|v and W1|W2 GEMMs: the switch, and -- with the guard armed -- the
        calibration of the current weights (calibrate_block_folds).  A caller with data in hand (`images` only says that the tower is about
        to run; its content does not enter the decision) that finds the weights uncalibrated calibrates them on the spot WITHOUT the
        collective: the probes are seeded, so ranks holding the same weights compute the same statistic up to device rounding; a job that
        wants the agreed value calls calibrate_block_folds() at a point every rank reaches (a warning says so in a multi-rank group)."""
        if not self.fold_block_ln:
            return False
        if not self.block_fold_guard:
            return True
        if self.block_fold_ratio is None:
            if images is None:
                return True
            if self._fold_group_active():
                import logging
                logging.warning("frozen tower: fold guard calibrated lazily inside a forward pass of a multi-rank job -- local value, no rank "
                                "agreement; call engine.calibrate_block_folds() on every rank after the weight load")
            self.calibrate_block_folds(collective=False)
        return self.block_fold_ratio <= self.block_fold_limit

    def _rccl_window_step(self, i, k0):
        """rccl_window = (leading blocks, CUs): the persistent GEMMs of the first chunk's leading blocks leave those CUs to RCCL's kernels
        (a prefetched pass runs them beside the student's gradient buckets)."""
        win, cus = self.rccl_window
        if win and k0 == 0 and i in (0, win) and hasattr(self.ops, "reserve_compute_units"):
            self.ops.reserve_compute_units(cus if i < win else 0)

    def _rccl_window_close(self, k0):
        """... and whatever happens inside the window (an exception included), the reservation does not outlive the pass."""
        if self.rccl_window[0] and k0 == 0 and hasattr(self.ops, "reserve_compute_units"):
            self.ops.reserve_compute_units(0)

    def _fold_pass(self, images) -> bool:
        """Does this encode_image() pass run the folded block schedule?  (May calibrate the guard: block_folds_active.)"""
        return self.block_folds_active(images)

    def _cls_block_folds(self) -> bool:
        return True

    def _identity_stats(self, M, C):
        """(mean = 0 [M], rstd = 1 [M], column sums = 0 [C]): statistics under which a folded-LayerNorm epilogue is the plain one, bit for bit."""
        key = ("ident", M, C)
        if key not in self._tables:
            self._tables[key] = (torch.zeros(M, dtype=F32, device=self.device), torch.ones(M, dtype=F32, device=self.device),
                                 torch.zeros(C, dtype=F32, device=self.device))
        return self._tables[key]

    def _resid_gemm_folded(self, A, W, bias, ln, x, xb, lo, part, first=False, last=False):
        """A residual GEMM of _teacher_block_folded: stream += LN(A) . W^T + bias with the LayerNorm folded -- ln = its (mean, rstd, column
        sums of gamma (.) W), or None where the family has no LayerNorm in front of this GEMM.  The stream is fp32 x, or with lo the planes
        (xb, lo): read from x by the first residual GEMM of the tower, written back to x by the last.  Every one but the last also leaves the
        bf16 copy xb of the new stream and the partial row statistics `part` for the next folded GEMM."""
        ops = self.ops
        if lo is not None:
            mean, rstd, colsum = ln if ln is not None else self._identity_stats(*x.shape)
            if last:
                ops.gemm_nt_ln_split(A, W, xb, lo, bias, mean, rstd, colsum, x_out=x)
            else:
                ops.gemm_nt_ln_split(A, W, xb, lo, bias, mean, rstd, colsum, x_in=x if first else None, stats_part=part)
        elif last and ln is None:                                       # nothing folded, nothing emitted: the plain residual GEMM
            ops.gemm_nt(A, W, x, bias=bias, extra=x, epi=EPI_RESID_F32)
        else:
            mean, rstd, colsum = ln if ln is not None else (None, None, None)
            ops.gemm_nt_ln(A, W, x, bias=bias, extra=x, ln_mean=mean, ln_rstd=rstd, ln_colsum=colsum, stats_part=None if last else part,
                           xb_out=None if last else xb, epi=EPI_RESID_LN_F32 if ln is not None else EPI_RESID_F32)

    def _row_stats(self, rows, keep):
        """(mean, rstd) buffers fp32 [rows] for a LayerNorm whose backward will run, else (None, None)."""
        return (self.ops.empty((rows,), F32), self.ops.empty((rows,), F32)) if keep else (None, None)

    def _teacher_qkv(self, i, x, xb, st, M):
        """q|k|v bf16 [M, 3C] of a _teacher_block_folded: the first block of the tower (xb None) runs the plain LayerNorm and GEMM on fp32 x,
        every later one the GEMM with the LayerNorm folded, on the bf16 copy xb and the statistics st the previous block left."""
        ops, C, n1 = self.ops, self.cfg.width, self._b(i) + self.NORM1
        qkv = ops.empty((M, 3 * C), BF16)
        if xb is None:
            ln1 = ops.empty((M, C), BF16)
            ops.layernorm_fwd(x, self.p[n1 + ".weight"], self.p[n1 + ".bias"], ln1, None, None, self.cfg.ln_eps)
            wqkv, bqkv = self._qkv_operands(i)
            ops.gemm_nt(ln1, wqkv, qkv, bias=bqkv, epi=EPI_BF16)
        else:
            Wq, cq, dq = self.fold[i]["qkv"]
            ops.gemm_nt_ln(xb, Wq, qkv, bias=dq, ln_mean=st[0], ln_rstd=st[1], ln_colsum=cq, epi=EPI_BF16)
        return qkv

    def _block_fwd_cls(self, i, x, B, N, cos, sin, xb=None, st=None, lo=None):
        """Last teacher block restricted to what encode_image() consumes: the CLS row.  x fp32 [B*N, C] -> fp32 [B, C].  The tower returns
        x[:, 0] after the final norm (eva_vit_model.py:505-519, transformer.py:486-494), so only the CLS *query* of the last block is live;
        keys and values still come from every token.  Row-for-row the same arithmetic as _block_fwd.
        With xb / st (/ lo) -- the bf16 operand view, first-LayerNorm statistics (and low plane) the previous folded block left -- that
        LayerNorm is folded into the K|V GEMM like in every other block of the tower (no LayerNorm pass over the 403 456-row stream, the
        stream never returns to fp32) and only the B CLS rows are rebuilt in fp32 for the query, the residual adds and the MLP."""
        ops, cfg = self.ops, self.cfg
        C, H, eps = cfg.width, cfg.heads, cfg.ln_eps
        n1 = self._b(i) + self.NORM1
        M = B * N
        wqkv, bqkv = self._qkv_operands(i)
        kv = ops.empty((M, 2 * C), BF16)
        q = ops.empty((B, C), BF16)
        if xb is not None:
            Wq, cq, dq = self.fold[i]["qkv"]
            ops.gemm_nt_ln(xb, Wq[C:], kv, bias=dq[C:], ln_mean=st[0], ln_rstd=st[1], ln_colsum=cq[C:], epi=EPI_BF16)
            xc = (self._join_planes(xb.view(B, N, C)[:, 0, :], lo.view(B, N, C)[:, 0, :]) if lo is not None
                  else x.view(B, N, C)[:, 0, :].contiguous())
            ln1c = ops.empty((B, C), BF16)
            ops.layernorm_fwd(xc, self.p[n1 + ".weight"], self.p[n1 + ".bias"], ln1c, None, None, eps)
            ops.gemm_nt(ln1c, wqkv[:C], q, bias=bqkv[:C], epi=EPI_BF16)
        else:
            ln1 = ops.empty((M, C), BF16)
            ops.layernorm_fwd(x, self.p[n1 + ".weight"], self.p[n1 + ".bias"], ln1, None, None, eps)
            ops.gemm_nt(ln1, wqkv[C:], kv, bias=bqkv[C:], epi=EPI_BF16)
            ops.gemm_nt(ln1.view(B, N, C)[:, 0, :], wqkv[:C], q, bias=bqkv[:C], epi=EPI_BF16)
            xc = x.view(B, N, C)[:, 0, :].contiguous()
        att = ops.empty((B, C), BF16)
        ops.attn_cls_fwd(q, kv, cos, sin, att, B, N, H, cfg.head_width ** -0.5)
        return self._block_tail(i, xc, att)

    def encode_image(self, images, chunk: int = 256):
        """Frozen-teacher path: full ViT, final LN on the CLS row, head.  [K,3,S,S] -> fp32 [K,E].
        Activation-free: crops are streamed in chunks, blocks update the residual stream in place."""
        ops, cfg, fn = self.ops, self.cfg, self.prefix + self.FINAL_NORM
        K = images.shape[0]
        out = ops.empty((K, cfg.embed_dim), F32)
        folded = self._fold_pass(images)
        for k0 in range(0, K, chunk):
            img = images[k0:k0 + chunk]
            B = img.shape[0]
            x, g = self._stem(img)
            N = g * g + 1
            cos, sin = self.rope_tables(g)
            xf = x.view(B * N, cfg.width)
            last = cfg.layers - 1 if self.cls_only_last_block else cfg.layers
            xb = st = None
            cls_folded = folded and self._cls_block_folds() and last < cfg.layers and last > 0      # the CLS-only block takes the planes + statistics as they are
            lo = ops.empty((B * N, cfg.width), torch.int16) if folded and self.split_stream and self._lo_plane(last, cls_folded) else None
            try:
                for i in range(last):
                    self._rccl_window_step(i, k0)
                    if folded:
                        xb, st = self._teacher_block_folded(i, xf, xb, st, B, N, cos, sin, emit_next=i + 1 < last or cls_folded, lo=lo)
                    else:
                        self._block_fwd(i, xf, B, N, cos, sin, True, None, True)
            finally:
                self._rccl_window_close(k0)
            if last < cfg.layers:
                xc = self._block_fwd_cls(last, xf, B, N, cos, sin, xb if cls_folded else None, st, lo)
            else:
                xc = x[:, 0, :]
            cls = ops.empty((B, cfg.width), BF16)
            ops.layernorm_fwd(xc, self.p[fn + ".weight"], self.p[fn + ".bias"], cls, None, None, cfg.ln_eps)
            self._head(cls, out[k0:k0 + B])
        return out

    # ------------------------------------------------------------------------------------------ student
    def _check_taps(self, taps, need_grad):
        """taps of encode_dense: a sorted tuple of distinct block indices in [0, L-1], on a frozen pass, on a backend that can copy them out."""
        L = self.cfg.layers
        taps = tuple(int(i) for i in taps)
        if need_grad:
            raise ValueError("encode_dense(taps=...) is the frozen detector-backbone pass: it cannot keep activations (need_grad=True)")
        if any(not 0 <= i < L for i in taps):
            raise ValueError(f"encode_dense(taps={taps}): block indices must lie in [0, {L - 1}] for this {L}-block tower")
        if any(b <= a for a, b in zip(taps, taps[1:])):
            raise ValueError(f"encode_dense(taps={taps}): block indices must be strictly ascending (the order the blocks run in)")
        if not getattr(self.ops, "TOKEN_TAPS", False):
            raise NotImplementedError(f"block taps (encode_dense(taps=...), forward_intermediates, the detector backbone) need the "
                                      f"tokens-to-[B, C, h, w] copy of the residual stream, which the kernel backend "
                                      f"{getattr(self.ops, 'name', type(self.ops).__name__)!r} does not provide (no TOKEN_TAPS)")
        return taps

    def encode_dense(self, images, need_grad: bool = False, taps=None, final: bool = True, tap_dtype=F32, tap_rows=()):
        """Dense path -> L2-normalised token map fp32 [B, N, E] (row 0 of each image is the unused CLS slot).
        With need_grad the activations of the trainable blocks (and of a trainable stem) are kept for backward_dense().
        taps (frozen pass only): block indices whose output -- the in-place residual stream after that block, index L-1 being the output of
        the last block's attention-free form -- is copied out as a [B, C, h, w] map (tap_dtype fp32 or bf16) before the next block
        overwrites it (F-ViT evaclip_vit.py:90-97); the method then returns (map, grid, [tap maps]).  final=False stops after the last
        block: no final LayerNorm, head or normalisation, None for the map (the backbone's training-mode branch, :98-106).
        tap_rows: positions within `taps` whose tap is delivered as neck.TokenRows instead of a map -- the whole stream [B*N, C], CLS
        rows included (off = 1), cast to bf16 by one cs_cast_f32_bf16 launch: the operand a Deconv2x2 contracts as it is."""
        ops, cfg, fn = self.ops, self.cfg, self.prefix + self.FINAL_NORM
        if taps is not None:
            taps = self._check_taps(taps, need_grad)
        tap_rows = tuple(int(k) for k in tap_rows)
        if tap_rows and (taps is None or any(not 0 <= k < len(taps) for k in tap_rows)):
            raise ValueError(f"encode_dense(tap_rows={tap_rows}): positions within taps={taps}")
        if need_grad and not final:
            raise ValueError("encode_dense(need_grad=True) differentiates the normalised map: final=False leaves nothing to differentiate")
        B = images.shape[0]
        stem_keep = {} if (need_grad and self._pos_trains()) else None
        x, g = self._stem(images, stem_keep)
        N, C, E = g * g + 1, cfg.width, cfg.embed_dim
        cos, sin = self.rope_tables(g)
        xf = x.view(B * N, C)
        saves = {}
        maps = []
        for i in range(cfg.layers):
            keep = need_grad and i >= self.first_trainable
            save = {} if keep else None
            xf = self._block_fwd(i, xf, B, N, cos, sin, with_attn=(i < cfg.layers - 1), save=save, inplace=not keep)
            if keep:
                saves[i] = save
            if taps is not None and i in taps:
                if len(maps) in tap_rows:
                    from .neck import TokenRows
                    assert xf.is_contiguous()
                    rows = ops.empty((B * N, C), BF16)
                    ops.cast_f32_bf16(xf, rows)
                    maps.append(TokenRows(rows, B, g, g, 1))
                else:
                    maps.append(ops.empty((B, C, g, g), tap_dtype))
                    ops.tokens_to_nchw(xf, B, N, C, maps[-1])
        if not final:
            return (None, g) if taps is None else (None, g, maps)
        M = B * N
        lnf = ops.empty((M, C), BF16)
        mean = ops.empty((M,), F32) if need_grad else None
        rstd = ops.empty((M,), F32) if need_grad else None
        ops.layernorm_fwd(xf, self.p[fn + ".weight"], self.p[fn + ".bias"], lnf, mean, rstd, cfg.ln_eps)
        feats = ops.empty((M, E), F32)
        self._head(lnf, feats)
        dense = ops.empty((M, E), F32)
        inv = ops.empty((M,), F32)
        ops.l2norm_fwd(feats, dense, inv)
        if need_grad:
            self._ctx = dict(B=B, N=N, g=g, saves=saves, xL=xf, stf=(mean, rstd), dense=dense, inv=inv, cos=cos, sin=sin, stem=stem_keep,
                             lnf=lnf if self.train_all else None)
        return (dense.view(B, N, E), g) if taps is None else (dense.view(B, N, E), g, maps)

    def roi_pool(self, dense, rois, g):
        """rois [K,5] = (image index, x0,y0,x1,y1 normalised to [0,1]) -> fp32 [K,E]."""
        pooled = self.ops.empty((rois.shape[0], dense.shape[2]), F32)
        if rois.shape[0]:
            self.ops.roialign_fwd(dense, rois, pooled, g, g, 1)
        return pooled

    # ------------------------------------------------------------------------------------------ backward
    def zero_grad(self):
        self.grad.zero_()

    def _wgrad(self, dY, X, dW):
        """dW[N,K] += dY^T X, dY [M,N] and X [M,K] token-major bf16.  cs_gemm_wgrad_tn contracts them as they are (transposing LDS
        reads); shapes it does not cover (N or K not a multiple of 8) go through explicit transposes + the NT split-K kernel."""
        ops = self.ops
        M, N = dY.shape
        K = X.shape[1]
        need = ops.gemm_wgrad_tn_workspace(N, K, M) if self.wgrad_tn else 0
        if need:
            if self._wgrad_ws is None or self._wgrad_ws.numel() < need:
                self._wgrad_ws = ops.empty((need,), torch.uint8)
            ops.gemm_wgrad_tn(dY, X, dW, self._wgrad_ws)
            return
        Xt = self._transposed(X)
        Mp = Xt.shape[1]
        dYt = ops.empty((N, Mp), BF16)
        ops.transpose_bf16(dY, dYt)
        need = ops.gemm_wgrad_workspace(N, Xt.shape[0], Mp)
        if self._wgrad_ws is None or self._wgrad_ws.numel() < need:
            self._wgrad_ws = ops.empty((need,), torch.uint8)
        ops.gemm_wgrad(dYt, Xt, dW, self._wgrad_ws)                      # split-K through partial buffers, then dW += sum

    def _transposed(self, X):
        M, K = X.shape
        Xt = self.ops.empty((K, _round_up(M, 64)), BF16)
        self.ops.transpose_bf16(X, Xt)
        return Xt

    def _bwd_gq(self, M):
        """(e4m3 codes, row scales) buffers for the bf16 copy of the stream gradient, or None (no fp8 dgrad)."""
        return None

    def _bwd_workspaces(self, M, B, N, Q=0):
        """ws of a backward pass over M rows: (LayerNorm-backward / attention-backward scratch, column-sum scratch), uint8.  Q: extra query
        rows per image in the attention backward (mask-attention pooling)."""
        ops = self.ops
        ln_width, colsum_width = self._bwd_widths()
        extra = (Q,) if Q else ()                     # (a backend without extra query rows takes no Q)
        ws_bytes = max(ops.layernorm_bwd_workspace(M, ln_width), ops.attn_bwd_workspace(B, N, self.cfg.heads, *extra))
        return ops.empty((ws_bytes,), torch.uint8), ops.empty((max(ops.colsum_workspace(M, colsum_width), 4),), torch.uint8)

    def _resid_bias(self, i):
        """Gradient slot of block i's second residual bias, None for a frozen block."""
        return self.g[self._b(i) + self.RESID_BIAS] if i >= self.first_trainable else None

    def _final_norm_bwd(self, c, d_feats, d_lnf, g, gb, ws, gq=None):
        """Head of a backward pass, from the context c of its forward: with train_all the head's weight gradient and the final norm's gamma /
        beta gradients (then the "head" bucket is complete); in either case g = the gradient w.r.t. the last block's output, assigned.  Its
        bf16 copy gb (and e4m3 copy gq), whose column sums are the last block's second residual bias gradient, is wanted when a block trains."""
        L, fn = self.cfg.layers, self.prefix + self.FINAL_NORM
        if self.train_all:
            self._head_wgrad(d_feats, c["lnf"], ws)
        dgamma, dbeta = (self.g[fn + ".weight"], self.g[fn + ".bias"]) if self.train_all else (None, None)
        copy = self.first_trainable < L
        q8a = dict(q8=gq[0], q_scale=gq[1]) if gq is not None and copy else {}
        self.ops.layernorm_bwd(d_lnf, c["xL"], self.p[fn + ".weight"], *c["stf"], g, DX_F32_ASSIGN, dgamma, dbeta, True, ws[0],
                               dx_copy=gb if copy else None, copy_colsum=self._resid_bias(L - 1), **q8a)
        if self.train_all and self.grad_ready_hook is not None:
            self.grad_ready_hook("head")

    def backward_dense(self, d_dense):
        """d_dense: fp32 [B, N, E] gradient w.r.t. the normalised token map (CLS rows zero).  Accumulates every trainable gradient into the
        flat grad buffer; fires grad_ready_hook("head" / block index / "stem") as buckets complete."""
        ops, cfg = self.ops, self.cfg
        c = self._ctx
        if c is None:
            raise RuntimeError("backward_dense() without a preceding encode_dense(need_grad=True)")
        self._ctx = None
        B, N, C, E = c["B"], c["N"], cfg.width, cfg.embed_dim
        M = B * N
        d_feats = ops.empty((M, E), BF16)
        ops.l2norm_bwd(d_dense.reshape(M, E), c["dense"], c["inv"], d_feats)
        d_lnf = ops.empty((M, C), BF16)
        self._head_dgrad(d_feats, d_lnf)
        g = ops.empty((M, C), F32)
        gb = ops.empty((M, C), BF16)                  # bf16 copy of g, written by the LayerNorm backwards that update g
        gq = self._bwd_gq(M)
        ws = self._bwd_workspaces(M, B, N)
        # (the CLS rows of d_feats are exact zeros -- the dense map drops them --, so they add nothing to any sum of the head's gradients)
        self._final_norm_bwd(c, d_feats, d_lnf, g, gb, ws, gq)
        for i in range(cfg.layers - 1, self.first_trainable - 1, -1):
            self._block_bwd(i, c["saves"].pop(i), g, gb, B, N, c["cos"], c["sin"], ws, next_bias=self._resid_bias(i - 1) if i > 0 else None, gq=gq)
            if self.grad_ready_hook is not None:
                self.grad_ready_hook(i)
        if c["stem"] is not None:
            self._stem_bwd(g, c["stem"], B, N, c["g"], ws[0])
            if self.grad_ready_hook is not None:
                self.grad_ready_hook("stem")

    def roi_pool_backward(self, d_pooled, rois, B, N, g):
        d_dense = self.ops.zeros((B, N, self.cfg.embed_dim), F32)
        if rois.shape[0]:
            self.ops.roialign_bwd(d_pooled.contiguous(), rois, d_dense, g, g, 1)
        return d_dense

    # ------------------------------------------------------------------------------------------ optimizer
    def adamw_step(self, step: int, lr: float, wd: float, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale: float = 1.0, max_norm=None,
                   skip_nonfinite: bool = False):
        """One flat AdamW launch over every trainable tensor (fp32 master + bf16 shadow refresh), then the W^T shadows.
        max_norm (a number; None or <= 0: no clipping) / skip_nonfinite: the guarded form of cs_adamw_step -- the L2 norm of grad_scale * grad
        over the active tensors is taken on the device, the gradient enters the update times min(1, max_norm / (norm + 1e-6)), and with
        skip_nonfinite a step whose norm is Inf or NaN writes nothing.  What follows the launch runs either way: after a skipped step it
        rewrites the derived copies from unchanged weights."""
        kw = {}
        if max_norm is not None or skip_nonfinite:
            if not getattr(self.ops, "ADAMW_GUARD", False):
                raise NotImplementedError(f"the '{self.ops.name}' backend has no guarded AdamW step (gradient clipping / non-finite-step skip on the device)")
            if self.guard is None:
                self.guard = self.ops.zeros((self.ops.adamw_guard_numel(self.numel),), F32)
            kw = dict(max_norm=float(max_norm or 0.0), skip_nonfinite=bool(skip_nonfinite), guard=self.guard)
        self.ops.adamw_step(self.master, self.grad, self.exp_avg, self.exp_avg_sq, self.shadow, self.flags,
                            lr, beta1, beta2, eps, wd, step, grad_scale, **kw)
        self.sync_transposed()
        if self._pos_trains():
            self._pos_cache.clear()                # the position table moved: drop the rescaled copies of non-native grids
