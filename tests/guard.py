"""Guard bands around device tensors: do the kernels stay inside their buffers?

The numeric tests cannot see a store a few elements past the end of a tensor (`torch.empty` and `engine.Arena` round sizes up to
256 / 512 bytes: the store lands in slack nobody reads) nor a read of memory that was never written (fresh device memory is zero).
Here every tensor a kernel sees is carved out of ONE backing buffer the test owns:

  GuardPool     tensors of any dtype for direct calls of the C entries: 256-byte aligned start, the last byte directly followed by
                canary bytes (sizes are NOT rounded), at least `guard` canary bytes on each side;
  GuardedArena  a drop-in for `lm_net_amd.engine.Arena` (`Engine.arena`, or `LM_Net.Arena` under plans): the production alignment,
                one whole 256-byte granule of canary between allocations; the padding inside an allocation's last granule and the
                unallocated rest of the arena are canary too.

`check()` compares every canary byte on the device in one masked comparison and names the damaged regions.  What this sees: writes
that leave a tensor and land within the canary next to it (or anywhere in unallocated arena).  What it cannot see: a far stray write
that lands inside ANOTHER tensor's body (left to the numeric tests), and reads -- those show only through their effect on results,
which is why the model tests run each configuration three times (ordinary allocations, poisoned bodies, junk bodies) and require
bit-identical results.  Poison is 0xFF bytes: NaN as fp32 and as either bf16 half, -1 as an integer, 255 as uint8.  The junk arena
instead holds finite, non-zero, sign-alternating values of the order 1e3 EVERYWHERE (v_max / v_min / clamps / selects return the
non-NaN operand, so a Hardswish or ReLU clamp can swallow a poisoned read; finite junk also survives 0 * x); its canaries are
compared against a pristine copy of the same pattern.  The junk is laid down once, before any launch, and not per allocation: a
fill enqueued at alloc time on the caller's stream would race with the kernels of the schedule's other streams.

Everything here is ordinary in-bounds tensor arithmetic on memory the process owns; nothing provokes a fault.  Importable without
a GPU (tests/test_guard_cpu.py exercises the layout and the detector on the CPU)."""
import bisect

import torch

GRANULE = 256                 # bytes: the production arena's alignment (engine.Arena: 64 floats)
POISON = 0xFF


def _numel(shape):
    n = 1
    for d in shape:
        n *= int(d)
    return n


def _itemsize(dtype):
    return torch.empty((), dtype=dtype).element_size()


class _Guarded:
    """Backing bytes + the list of carved tensors + the detector."""

    def _init(self, raw, ref):
        self.raw = raw                      # uint8 view of the whole backing buffer
        self.ref = ref                      # uint8 pristine copy (junk pattern), or None: canaries are POISON
        self.mask = torch.ones_like(raw)    # 1 = canary byte
        self.entries = []                   # (name, first byte, bytes)
        self._masked = 0                    # entries already cleared from the mask

    def _sync(self):
        if self.raw.is_cuda:
            torch.cuda.synchronize(self.raw.device)

    def guard_bytes(self):
        return self.raw.numel() - sum(e[2] for e in self.entries)

    def check(self):
        """-> [(tensor name, "before" | "after", first, last)]: damaged canary bytes, offsets relative to the END of the named tensor
        (after: 0 is the first byte past the end; before: negative, below -size).  A gap between two tensors is split in the middle."""
        self._sync()
        for _, a, nb in self.entries[self._masked:]:
            if nb:
                self.mask[a:a + nb] = 0
        self._masked = len(self.entries)
        n, step, idx = self.raw.numel(), 1 << 28, []
        for lo in range(0, n, step):                          # (each chunk is reduced to its damaged indices and dropped at once)
            hi = min(n, lo + step)
            want = self.ref[lo:hi] if self.ref is not None else POISON
            bad = (self.raw[lo:hi] != want) & (self.mask[lo:hi] != 0)
            if bool(bad.any()):
                idx += [int(i) + lo for i in bad.nonzero().flatten().cpu().tolist()]
            del bad
        if not idx:
            return []
        starts = [e[1] for e in self.entries]
        out = {}
        for i in idx:
            k = bisect.bisect_right(starts, i) - 1            # last tensor starting at or before byte i
            if k < 0:
                k, side = 0, "before"
            elif k + 1 < len(self.entries):
                end = starts[k] + self.entries[k][2]
                side = "after" if i - end < starts[k + 1] - i else "before"
                k = k if side == "after" else k + 1
            else:
                side = "after"
            if not self.entries:
                key, rel = ("<empty>", "after"), i
            else:
                name, a, nb = self.entries[k]
                key, rel = (name, side), i - (a + nb)
            lo_hi = out.get(key)
            out[key] = (rel, rel) if lo_hi is None else (min(lo_hi[0], rel), max(lo_hi[1], rel))
        return [(k[0], k[1], v[0], v[1]) for k, v in out.items()]

    def assert_clean(self, where=""):
        bad = self.check()
        if bad:
            raise AssertionError("guard bytes damaged%s: %s" % (" " + where if where else "", "; ".join(
                "%s %s [%+d .. %+d]" % b for b in bad)))


class GuardPool(_Guarded):
    """Tensors for ONE direct call of a C entry: inputs, outputs, parameter tables and workspace, each flush against canaries."""

    def __init__(self, device, nbytes, guard=4096):
        self.guard = int(guard)
        self.nbytes = (int(nbytes) + GRANULE - 1) // GRANULE * GRANULE
        self.buf = torch.full((self.nbytes,), POISON, dtype=torch.uint8, device=device)
        self._init(self.buf, None)
        self.off = 0                        # first free byte
        self.t = {}                         # name -> tensor
        self.inputs = {}                    # name -> copy taken at take()

    def take(self, name, shape, dtype=torch.float32, init=None):
        if init is not None:
            shape, dtype = tuple(init.shape), init.dtype
        shape = tuple(int(d) for d in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
        nb = _numel(shape) * _itemsize(dtype)
        a = (self.off + self.guard + GRANULE - 1) // GRANULE * GRANULE
        if a + nb + self.guard > self.nbytes:
            raise RuntimeError("GuardPool exhausted (%d + %d + %d > %d bytes)" % (a, nb, self.guard, self.nbytes))
        if name in self.t:
            raise KeyError("GuardPool: %r taken twice" % (name,))
        t = self.buf[a:a + nb].view(dtype).view(shape)
        self.entries.append((name, a, nb))
        self.off = a + nb
        self.t[name] = t
        if init is not None:
            t.copy_(init)
            self.inputs[name] = t.clone()
        return t

    def alloc(self, device, shape, dtype=torch.float32):
        """Signature of `hip._ALLOC[0]` / `Engine.alloc`: the library wrappers' own allocations (deferred K-split workspaces, ...)."""
        return self.take("alloc%d %s" % (len(self.entries), tuple(shape)), shape, dtype)

    def unchanged(self, name):
        """Does the tensor registered as an input (take(init=...)) still hold what was copied in?  Compared as bytes: NaN-safe."""
        self._sync()
        return torch.equal(self.t[name].contiguous().view(torch.uint8).flatten(), self.inputs[name].view(torch.uint8).flatten())

    def assert_inputs_unchanged(self, skip=()):
        bad = [k for k in self.inputs if k not in skip and not self.unchanged(k)]
        assert not bad, "inputs changed by the call: %s" % bad

    @staticmethod
    def size_for(tensors_bytes, guard=4096):
        """Bytes a pool needs for tensors of the given byte sizes."""
        return sum((nb + guard + 2 * GRANULE) for nb in tensors_bytes) + guard + GRANULE


JUNK = 0xA5


def pools(inputs, outputs, device, fill):
    """(plain tensors, GuardPool, guarded tensors) for one direct call of a C entry, run once on each side: `inputs` name -> tensor,
    copied in; `outputs` name -> (shape, dtype).  The pool holds every tensor at its exact size.  fill="junk": every output byte on
    both sides is JUNK (an entry that writes all of its outputs: whatever it leaves shows).  fill="poison": the plain uint8 outputs
    hold POISON as the pool's bodies do, the other plain outputs are uninitialised (an entry that writes part of a uint8 case buffer:
    the test compares the untouched part)."""
    if fill not in ("junk", "poison"):
        raise ValueError("pools: fill is 'junk' or 'poison', got %r" % (fill,))
    plain = {k: v.to(device) for k, v in inputs.items()}
    plain.update({k: torch.empty(s, dtype=dt, device=device) for k, (s, dt) in outputs.items()})
    pool = GuardPool(device, GuardPool.size_for([v.numel() * v.element_size() for v in plain.values()]))
    guarded = {k: pool.take(k, None, None, init=v.to(device)) for k, v in inputs.items()}
    guarded.update({k: pool.take(k, s, dt) for k, (s, dt) in outputs.items()})
    for d in (plain, guarded):
        for k, (_, dt) in outputs.items():
            if fill == "junk":
                d[k].view(torch.uint8).fill_(JUNK)
            elif dt == torch.uint8:
                d[k].fill_(POISON)
    return plain, pool, guarded


def sizes(pool, plain):
    """name -> bytes of every tensor of the pool, asserted equal to the plain tensors' sizes: nothing is rounded up."""
    got = {e[0]: e[2] for e in pool.entries}
    assert got == {k: v.numel() * v.element_size() for k, v in plain.items()}
    return got


def junk_pattern(device):
    """128 fp32 values (two granules) that are finite, non-zero and of the order 1e3 both as fp32 and as either bf16 half; the fp32
    signs alternate, the bf16 signs go + + - -.  1024 + 8 k is exact in bf16."""
    j = torch.arange(256, dtype=torch.int64)
    mag = 1024.0 + 8.0 * ((j * 37) % 128).double()
    sign = 1.0 - 2.0 * ((j // 2) % 2).double()
    return (mag * sign).to(torch.bfloat16).to(device)


class GuardedArena(_Guarded):
    """Drop-in for `lm_net_amd.engine.Arena` (same `alloc(shape, dtype)`, same `buf` / `off` in floats) with a canary granule after
    every allocation.  `count` / `used` (floats inside allocations, as Engine.alloc_floats counts them) size it: the floats of an
    ordinary pass plus `floats_for(...)`'s one granule per allocation."""

    def __init__(self, nfloats, device, body="nan"):
        assert body in ("nan", "junk"), body
        nfloats = (int(nfloats) + 127) // 128 * 128
        self.body = body
        if body == "nan":
            self.buf = torch.full((nfloats,), float("nan"), dtype=torch.float32, device=device)
            self.buf.view(torch.uint8).fill_(POISON)
            ref = None
        else:
            self.buf = torch.empty(nfloats, dtype=torch.float32, device=device)
            self.buf.view(torch.bfloat16).view(-1, 256).copy_(junk_pattern(device))
            ref = self.buf.clone().view(torch.uint8)
        self._init(self.buf.view(torch.uint8), ref)
        self.off = 64                       # floats; the first granule is canary
        self.count = 0
        self.used = 0

    @staticmethod
    def floats_for(alloc_floats, nalloc):
        """Arena size for `nalloc` allocations totalling `alloc_floats` (Engine.alloc_floats: already rounded to granules)."""
        return int(alloc_floats) + 64 * (int(nalloc) + 2)

    def alloc(self, shape, dtype=torch.float32):
        shape = tuple(int(d) for d in shape)
        n = _numel(shape)
        nf = n if dtype == torch.float32 else (n + 1) // 2      # floats covering n elements (engine.Arena)
        n_al = (nf + 63) & ~63
        if self.off + n_al + 64 > self.buf.numel():
            raise RuntimeError("lm_net_amd: plan arena exhausted (%d + %d > %d floats) [guarded]" % (self.off, n_al + 64, self.buf.numel()))
        v = self.buf[self.off:self.off + nf]
        v = v.view(shape) if dtype == torch.float32 else v.view(dtype)[:n].view(shape)
        self.entries.append(("#%d %s %s" % (self.count, shape, str(dtype).replace("torch.", "")), 4 * self.off, n * _itemsize(dtype)))
        self.off += n_al + 64
        self.count += 1
        self.used += n_al
        return v


def pollute_allocator(device, body="nan"):
    """Leave poison (0xFF) or junk in the blocks torch's caching allocator will hand out next: tensors of many sizes are filled and
    freed, so that a later `torch.empty` -- the buffers the library's wrappers and the modules around the model allocate for
    themselves, outside `Engine.alloc` -- no longer starts from the zeros of fresh device memory.  A long training process is in this
    state all the time; a fresh test process never is."""
    keep = []
    pat = junk_pattern(device) if body == "junk" else None
    for nbytes, cnt in ((512, 4000), (4096, 2000), (65536, 600), (1 << 20, 300), (16 << 20, 40), (256 << 20, 6)):
        for _ in range(cnt):
            t = torch.empty(nbytes, dtype=torch.uint8, device=device)
            if pat is None:
                t.fill_(POISON)
            else:
                t.view(torch.bfloat16).view(-1, 256).copy_(pat)
            keep.append(t)
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize(device)
    del keep


class LaunchLog:
    """Context manager around `hip._check`: records the name of every C entry issued through the Python wrappers (`names`), and --
    given an arena or pool -- synchronises after every launch (run the serial schedule for this: `branch_overlap=False,
    overlap_wgrad=False`) and

      * runs `check()`, raising at the FIRST entry after which the canaries are no longer clean (a write past a tensor);
      * with trace=True (GuardedArena only) keeps, per launch, a digest of every allocation's body and how many of its 32-bit words
        still hold the prefill.  `LaunchLog.first_divergence(a, b)` compares the traces of the same pass in a poisoned and in a
        junk arena: the first launch whose OUTPUT differs between the two consumed memory nobody had written -- it names that launch,
        the tensor that differs and the arena tensors that still held prefill words at that moment (the candidates it read).

    A debugging aid for a tripped guard or a fill that changes a result; these are reads and writes inside the process's own
    allocation, not memory faults."""

    def __init__(self, guarded=None, trace=False):
        self.guarded = guarded
        self.trace = [] if trace else None          # per launch: (what, entries so far, digests int64[n], prefill words int64[n])
        self.names = []

    def _digest(self):
        g = self.guarded
        torch.cuda.synchronize() if g.raw.is_cuda else None
        w = g.raw.view(torch.int32)
        pristine = (w == (g.ref.view(torch.int32) if g.ref is not None else -1))
        cs = torch.cat([w.new_zeros(1, dtype=torch.int64), torch.cumsum(torch.where(pristine, 0, w).long(), 0)])
        cp = torch.cat([w.new_zeros(1, dtype=torch.int64), torch.cumsum(pristine.long(), 0)])
        lo = torch.tensor([a // 4 for _, a, _ in g.entries], dtype=torch.int64, device=w.device)
        hi = torch.tensor([(a + nb + 3) // 4 for _, a, nb in g.entries], dtype=torch.int64, device=w.device)
        return (cs[hi] - cs[lo]).cpu(), (cp[hi] - cp[lo]).cpu()

    def __enter__(self):
        from lm_net_amd import hip
        self._hip, self._orig = hip, hip._check

        def _check(rc, what):
            self._orig(rc, what)
            self.names.append(what)
            if self.guarded is not None:
                self.guarded.assert_clean("after launch #%d (%s)" % (len(self.names), what))
                if self.trace is not None:
                    self.trace.append((what, len(self.guarded.entries)) + self._digest())
        hip._check = _check
        return self

    def __exit__(self, *exc):
        self._hip._check = self._orig
        return False

    @staticmethod
    def first_divergence(a, b):
        """a, b: LaunchLog(arena, trace=True) of the SAME pass in two arenas with different prefill -> None, or (launch number, entry
        name, [tensors that differ], [tensors allocated by then that still held prefill words before the launch])."""
        for i, ((wa, na, da, pa), (wb, nb, db, pb)) in enumerate(zip(a.trace, b.trace)):
            assert wa == wb and na == nb, ("the two passes issue different launches", i, wa, wb)
            words = [(e[2] + 3) // 4 for e in a.guarded.entries[:na]]
            # compare what has been written completely in both runs (a partly written body mixes in the prefill, which differs by design)
            diff = [k for k in range(na) if int(pa[k]) == 0 and int(pb[k]) == 0 and int(da[k]) != int(db[k])]
            if diff:
                prev = a.trace[i - 1][3] if i else pa
                stale = [a.guarded.entries[k][0] for k in range(min(na, len(prev))) if 0 < int(prev[k]) and words[k]]
                return i + 1, wa, [a.guarded.entries[k][0] for k in diff], stale
        return None


# ---------------------------------------------------------------------------------------------------------------- coverage manifest
MODEL = "tests/test_guard_model_gpu.py"
KERN = "tests/test_guard_kernels_gpu.py"
ONEOF = "tests/test_guard_oneof_gpu.py"
LOSS = "tests/test_guard_loss_gpu.py"
SIGMOID = "tests/test_guard_sigmoid_gpu.py"
OPTIM, TILES, CURVES, VOLUME, VOLPOST, LESION, DISTMAP, LOVASZ, REGION, SLICES, SOFT, HARD = (
    "tests/test_guard_%s_gpu.py" % x for x in ("optim", "tiles", "curves", "volume", "volpost", "lesion", "distmap", "lovasz", "region", "slices", "soft", "hard"))


def _fam(*wrappers):
    """entries of the kernel_checks.py families: lmn_<wrapper>, guarded by test_model_kernel_families (which asserts it reached them)"""
    return {"lmn_" + w: (KERN, "test_model_kernel_families", w) for w in wrappers}


# C entry -> (test file, test function, `hip.` wrapper through which that test issues the entry).  tests/test_guard_cpu.py checks that
# this and EXEMPT partition hip.EXPORTS (every header's list) and that the named test's file calls `hip.<wrapper>` -- or, where the
# test reaches the entry through a class of the package, asserts the wrapper's name in its launch log: a new export needs a guard test.
# A new header joins here: its device entries in COVERED with a guard test of their own, the rest in EXEMPT with the reason.
# (The engine-allocated side of the same entries -- every intermediate of the model's own pass -- is tests/test_guard_model_gpu.py.)
COVERED = dict(_fam(
    "conv_fwd", "conv_wgrad", "reparam_fold", "reparam_wfin", "affine2", "bnact_fwd_fin", "bnact_bwd_fin",
    "dw_stats", "dw_fwd", "dw_merge", "dw_finalize_merge", "dw_bwd_stats", "dw_bwd_coef", "dw_bwd", "dw_fwd_bn", "dw_bwd_bn",
    "se_fwd", "se_bwd", "se_bwd_dm", "se_bwd_params", "na_fwd", "na_bwd", "gattn_fwd", "gattn_bwd", "ln_fwd", "ln_bwd",
    "bnact_fwd", "bnact_bwd_stats", "bnact_bwd", "bn_finalize", "bn_bwd_coef", "up2_fwd", "up2_bwd", "avgpool_fwd", "avgpool_bwd"))
COVERED.update({
    "lmn_wgrad_reduce_batch": (KERN, "test_model_kernel_families", "wgrad_reduce_flush"),
    "lmn_conv_pack": (KERN, "test_conv_pack_exact_size_feeds_conv_fwd", "conv_pack"),
    "lmn_conv_pack_batch": (KERN, "test_conv_pack_exact_size_feeds_conv_fwd", "PackPlan"),
    "lmn_bn_fold": (KERN, "test_bn_fold", "bn_fold"),
    "lmn_segloss_fwd": (KERN, "test_segloss_and_confusion", "segloss_fwd"),
    "lmn_segloss_bwd": (KERN, "test_segloss_and_confusion", "segloss_bwd"),
    "lmn_confusion": (KERN, "test_segloss_and_confusion", "confusion"),
    "lmn_confusion_labels": (KERN, "test_segloss_and_confusion", "confusion_labels"),
    "lmn_adamw_step": (KERN, "test_adamw_step", "adamw_step"),
    "lmn_fill": (KERN, "test_flat_utilities", "fill"),
    "lmn_add": (KERN, "test_flat_utilities", "add"),
    "lmn_colsum": (KERN, "test_strided_utilities", "colsum"),
    "lmn_copy_slice": (KERN, "test_strided_utilities", "copy_slice"),
    "lmn_copy2d": (KERN, "test_strided_utilities", "copy2d"),
    "lmn_nchw_to_nhwc": (KERN, "test_layout_conversions", "nchw_to_nhwc"),
    "lmn_nhwc_to_nchw": (KERN, "test_layout_conversions", "nhwc_to_nchw"),
    "lmn_preprocess_u8": (KERN, "test_preprocess_u8", "preprocess_u8"),
    "lmn_preprocess_u8_ex": (KERN, "test_preprocess_u8", "preprocess_u8_ex"),
    "lmn_augment_u8": (KERN, "test_augment_u8_ragged_batch", "augment_u8"),
    "lmn_surface_dist": (KERN, "test_surface_dist", "surface_dist"),
    "lmn_cc_label": (KERN, "test_post_clean_render_and_cc_label", "cc_label"),
    "lmn_post_clean": (KERN, "test_post_clean_render_and_cc_label", "post_clean"),
    "lmn_post_render": (KERN, "test_post_clean_render_and_cc_label", "post_render"),
    "lmn_augment_oneof_u8": (ONEOF, "test_augment_oneof_u8_every_member", "augment_oneof_u8"),
    "lmn_segloss_ex_fwd": (LOSS, "test_loss_and_image_stats_entries", "segloss_ex_fwd"),
    "lmn_segloss_ex_bwd": (LOSS, "test_loss_and_image_stats_entries", "segloss_ex_bwd"),
    "lmn_image_stats": (LOSS, "test_loss_and_image_stats_entries", "image_stats"),
    "lmn_sigloss_fwd": (SIGMOID, "test_loss_and_stats_entries", "sigloss_fwd"),
    "lmn_sigloss_bwd": (SIGMOID, "test_loss_and_stats_entries", "sigloss_bwd"),
    "lmn_sigmoid_stats": (SIGMOID, "test_loss_and_stats_entries", "sigmoid_stats"),
    "lmn_optim_prepare": (OPTIM, "test_prepare_and_step_entries", "optim_prepare"),
    "lmn_adamw_step_ex": (OPTIM, "test_prepare_and_step_entries", "adamw_step_ex"),
    "lmn_tile_gather": (TILES, "test_gather_and_blend_entries", "tile_gather"),
    "lmn_tile_blend": (TILES, "test_gather_and_blend_entries", "tile_blend"),
    "lmn_curve_hist": (CURVES, "test_curve_hist_entry", "curve_hist"),
    "lmn_volume_labels": (VOLUME, "test_volume_labels_entry", "volume_labels"),
    "lmn_volume_dist": (VOLUME, "test_volume_dist_entry", "volume_dist"),
    "lmn_cc3d_label": (VOLPOST, "test_cc3d_label_entry", "cc3d_label"),
    "lmn_volpost_clean": (VOLPOST, "test_volpost_clean_entry", "volpost_clean"),
    "lmn_lesion_match": (LESION, "test_lesion_match_entry", "lesion_match"),
    "lmn_dist_map": (DISTMAP, "test_dist_map_entry", "dist_map"),
    "lmn_dist_loss_fwd": (DISTMAP, "test_dist_loss_entries", "dist_loss_fwd"),
    "lmn_dist_loss_bwd": (DISTMAP, "test_dist_loss_entries", "dist_loss_bwd"),
    "lmn_lovasz_order": (LOVASZ, "test_lovasz_order_entry", "lovasz_order"),
    "lmn_lovasz_fwd": (LOVASZ, "test_lovasz_loss_entries", "lovasz_fwd"),
    "lmn_lovasz_bwd": (LOVASZ, "test_lovasz_loss_entries", "lovasz_bwd"),
    "lmn_region_fwd": (REGION, "test_region_loss_entries", "region_fwd"),
    "lmn_region_bwd": (REGION, "test_region_loss_entries", "region_bwd"),
    "lmn_slices_stats": (SLICES, "test_slices_entries", "slices_stats"),
    "lmn_slices_gather": (SLICES, "test_slices_entries", "slices_gather"),
    "lmn_soft_fwd": (SOFT, "test_soft_loss_entries", "soft_fwd"),
    "lmn_soft_bwd": (SOFT, "test_soft_loss_entries", "soft_bwd"),
    "lmn_mix_batch": (SOFT, "test_mix_batch_entry", "mix_batch"),
    "lmn_hard_fwd": (HARD, "test_hard_entries", "hard_fwd"),
    "lmn_hard_bwd": (HARD, "test_hard_entries", "hard_bwd"),
})

# The files under the strict rule -> what the named test function must hold besides: it CALLS `hip.<wrapper>(` AND compares a
# LaunchLog's `names` with a list that holds the wrapper (the general rule accepts either), and it runs the entry on a guard pool --
# these words.  (The AdamW step updates its inputs in place: its test carves the workspace at exactly hip.optim_workspace(n) instead.)
_POOL, _POOLS = ("GuardPool", "assert_clean", "assert_inputs_unchanged"), ("pools(", "assert_clean", "assert_inputs_unchanged")
STRICT = {LOSS: _POOL, SIGMOID: _POOL, OPTIM: ("GuardPool", "assert_clean", "hip.optim_workspace(n)"), TILES: _POOL, CURVES: _POOL, VOLUME: _POOLS, VOLPOST: _POOLS,
          LESION: _POOLS, DISTMAP: _POOLS, LOVASZ: _POOLS, REGION: _POOLS, SLICES: _POOLS, SOFT: _POOLS, HARD: _POOLS}

# entries that take no device output pointer -> why no guard test applies
_HOST = "host arithmetic only: returns a number, touches no device memory"
EXEMPT = {
    "lmn_abi_version": _HOST, "lmn_last_error": "returns the host-side error string",
    "lmn_sizeof_conv_args": _HOST, "lmn_sizeof_src": _HOST, "lmn_sizeof_wgrad_args": _HOST, "lmn_sizeof_pack_job": _HOST,
    "lmn_sizeof_reduce_job": _HOST, "lmn_sizeof_aug_param": _HOST, "lmn_sizeof_post_param": _HOST,
    "lmn_sizeof_oneof_param": _HOST, "lmn_sizeof_loss_param": _HOST, "lmn_sizeof_sig_param": _HOST,
    "lmn_conv_pack_size": _HOST + " (tested AS A BOUND by test_conv_pack_exact_size_feeds_conv_fwd)",
    "lmn_conv_wgrad_workspace": _HOST + " (tested as a bound by test_model_kernel_families: hip._workspace returns exactly this)",
    "lmn_surface_workspace": _HOST + " (tested as a bound by test_surface_dist)",
    "lmn_post_workspace": _HOST + " (tested as a bound by test_post_clean_render_and_cc_label)",
    "lmn_oneof_workspace": _HOST + " (tested as a bound by test_augment_oneof_u8_every_member: the workspace is carved at exactly this)",
    "lmn_sizeof_optim_param": _HOST, "lmn_sizeof_tile_param": _HOST,
    **{"lmn_%s_workspace" % x: _HOST + " (tested as a bound by %s: the workspace is carved at exactly this)" % test for x, test in (
        ("optim", "test_prepare_and_step_entries"), ("curve", "test_curve_hist_entry"), ("volume", "test_volume_dist_entry"),
        ("volpost", "test_volpost_clean_entry"), ("lesion", "test_lesion_match_entry"), ("dist", "test_dist_map_entry"),
        ("lovasz", "test_lovasz_order_entry"), ("region", "test_region_loss_entries"), ("slices", "test_slices_entries"),
        ("soft", "test_soft_loss_entries"), ("hard", "test_hard_entries"))},
    "lmn_conv_chain_ok": "launch predicate, " + _HOST, "lmn_conv_wgrad_up2_ok": "launch predicate, " + _HOST,
    "lmn_conv_wgrad_job": "geometry query into a host struct, " + _HOST,
    "lmn_conv_dma_config": "process-wide dispatch switch, host state only",
    "lmn_stream_wait": "stream ordering, no data", "lmn_event_record": "stream ordering, no data",
    "lmn_event_wait": "stream ordering, no data", "lmn_set_priority_stream": "host-side table of stream priorities",
    "lmn_set_deterministic": "process-wide switch, host state only", "lmn_get_deterministic": "process-wide switch, host state only",
    "lmn_plan_create": "plan recorder: host memory only", "lmn_plan_destroy": "plan recorder: host memory only",
    "lmn_plan_record_begin": "plan recorder: host memory only", "lmn_plan_record_end": "plan recorder: host memory only",
    "lmn_plan_size": "plan recorder: host memory only",
    "lmn_plan_run": "re-issues recorded entries on their recorded pointers (guarded as a whole by test_plans_inside_guarded_arena)",
    "lmn_plan_host_profile": "runs a plan once and writes a HOST text buffer",
    "lmn_prof_begin": "kernel timer: host records only", "lmn_prof_end": "kernel timer: writes a HOST text buffer",
}
