"""Input pipelines: the host prefetcher, and the DIV2K, HisFrag and Michigan pipelines on the device
(DESIGN.md sections 16-18) - resident images, the per-batch random plans (pinned bit for bit against Pillow, cv2 and torchvision)
and the loaders that drive the feed kernels - and, on Pillow's resize at any scale, the Pajigsaw loader and
the evaluation sources of michigan.py and hisfrag.py."""
from __future__ import annotations

import collections
import math
from typing import NamedTuple

import torch

from .. import ops


class DevicePrefetcher:
    """Wraps a loader of (samples, targets) CPU batches.  The reference copies every batch on the compute stream at the top of
    the iteration (``samples.cuda(non_blocking=True)``, misc/engine.py:203-204) as fp32.  Here the batch is staged in pinned host
    memory and copied on a side stream ``depth`` batches ahead of the step that consumes it, and uint8 images stay uint8 all the
    way into the patch-embedding kernel (``vited_patchify_u8`` applies ToTensor + Normalize), so a config-A batch of 1024 pairs
    is 25 MB on PCIe instead of 101 MB.  Yields device tensors; iteration order and contents equal the wrapped loader's."""

    def __init__(self, loader, device, depth: int = 2):
        self.loader, self.device, self.depth = loader, torch.device(device), max(int(depth), 1)
        self.stream = torch.cuda.Stream(device=self.device) if self.device.type == 'cuda' else None
        self._pinned = {}

    def __len__(self):
        return len(self.loader)

    def _stage(self, t, slot, name):
        """CPU tensor -> device tensor through a reusable pinned buffer (per ring slot), on the copy stream."""
        if not torch.is_tensor(t):
            return t
        if self.stream is None:
            return t.to(self.device)
        key = (slot, name, tuple(t.shape), t.dtype)
        ent = self._pinned.get(key)
        if ent is None:
            ent = self._pinned[key] = [torch.empty(t.shape, dtype=t.dtype).pin_memory(), None]
        buf, ev = ent
        if ev is not None:
            ev.synchronize()               # the previous H2D copy out of this pinned slot must have executed before it is rewritten
        buf.copy_(t)
        out = buf.to(self.device, non_blocking=True)
        ent[1] = torch.cuda.Event()
        ent[1].record(self.stream)
        return out

    def __iter__(self):
        queue = collections.deque()
        slot = 0
        for batch in self.loader:
            samples, targets = batch
            if self.stream is not None:
                with torch.cuda.stream(self.stream):
                    item = (self._stage(samples, slot, 'x'), self._stage(targets, slot, 'y'))
                    ev = torch.cuda.Event()
                    ev.record(self.stream)
            else:
                item, ev = (self._stage(samples, slot, 'x'), self._stage(targets, slot, 'y')), None
            queue.append((item, ev))
            slot = (slot + 1) % (self.depth + 1)          # a pinned buffer is rewritten only after its batch was handed out
            if len(queue) > self.depth:
                yield self._hand_out(*queue.popleft())
        while queue:
            yield self._hand_out(*queue.popleft())

    def _hand_out(self, item, ev):
        if ev is not None:
            cur = torch.cuda.current_stream(self.device)
            cur.wait_event(ev)                              # the consumer's stream waits for the copy, the host does not
            for t in item:
                if torch.is_tensor(t):
                    t.record_stream(cur)
        return item


def div2k_pair_plan(u: torch.Tensor, img_size: int, erosion_ratio: float, with_negative: bool = True, train: bool = True):
    """The random choices of ``DIV2KPatch.__getitem__`` (div2k_patch.py:114-153) for a whole batch at once, from uniform numbers
    ``u`` [B, 4] in [0, 1) (columns: negative-pair draw, first swap, second swap, erosion):
      cells  int32 [B, 2]   grid cells (3 columns x 2 rows, row-major) of image 1 and image 2
      labels fp32  [B, 4]   the 4-bin target (all-zero for the 30 % negatives)
      erode  int32 [B]      eroded cell size e = ceil(S (1 - r)), r ~ U(erosion_ratio, 2 erosion_ratio) in training
    first = cell 0, second = 1 (right of it), third = 4 (below second), fourth = 3 (below first), spare = 2."""
    dev = u.device
    a, b = u[:, 1] > 0.5, u[:, 2] > 0.5
    neg = (u[:, 0] < 0.3) if with_negative else torch.zeros_like(a)
    second = torch.where(neg, torch.where(a, 4, 2), torch.where(a, 3, 1))      # negative: third / spare; positive: fourth / second
    first = torch.zeros_like(second)
    img1 = torch.where(b, second, first)
    img2 = torch.where(b, first, second)
    cells = torch.stack([img1, img2], dim=1).to(torch.int32)
    bin_ = a.long() + 2 * b.long()                                              # (a, b) -> label bin 0, 1, 2, 3
    labels = torch.nn.functional.one_hot(bin_, 4).float() * (~neg).float().unsqueeze(1)
    r = erosion_ratio * (1.0 + u[:, 3].double()) if train else torch.full_like(u[:, 3], erosion_ratio, dtype=torch.float64)
    erode = torch.ceil(img_size * (1.0 - r)).to(torch.int32).clamp_(1, img_size)
    return cells.contiguous(), labels.to(dev), erode.contiguous()


def assemble_pairs(regions_u8: torch.Tensor, cells: torch.Tensor, erode: torch.Tensor, img_size: int) -> torch.Tensor:
    """uint8 regions [B, C, 2 S, 3 S] on the device -> uint8 pairs [B, 2, C, S, S]: erosion crop + Pillow-exact bilinear resize of
    the two chosen cells in one kernel (``vited_crop_pairs_u8``).  Feed the result straight to the model: ToTensor + Normalize
    are folded into the patch-embedding kernel."""
    return ops.crop_pairs_u8(regions_u8, cells, erode, img_size)


class Div2kImageStore:
    """The decoded images of a DIV2K split, resident on ``device``: ``images`` (HWC uint8 arrays or tensors, 3 channels) packed
    back to back into one uint8 buffer (``data``), with their byte offsets and (H, W) sizes on the device (``offsets_dev`` int64
    [n], ``sizes_dev`` int32 [n, 2]) and on the host (``offsets``, ``sizes``).  DIV2K train is about 7 GB this way."""

    def __init__(self, images, device):
        self.device = torch.device(device)
        flat, sizes, offsets, off = [], [], [], 0
        for k, im in enumerate(images):
            t = torch.as_tensor(im)
            if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3 or t.shape[0] < 1 or t.shape[1] < 1:
                raise ValueError(f'image {k}: expected a uint8 [H, W, 3] array, got {t.dtype} {tuple(t.shape)}')
            flat.append(t.contiguous().reshape(-1))
            sizes.append([t.shape[0], t.shape[1]])
            offsets.append(off)
            off += t.numel()
        if not flat:
            raise ValueError('an image store needs at least one image')
        self.sizes = torch.tensor(sizes, dtype=torch.int32)
        self.offsets = torch.tensor(offsets, dtype=torch.int64)
        self.data = torch.empty(off, dtype=torch.uint8, device=self.device)
        for t, o in zip(flat, offsets):                    # image by image: no second host copy of the whole set
            self.data[o: o + t.numel()].copy_(t)
        self.sizes_dev, self.offsets_dev = self.sizes.to(self.device), self.offsets.to(self.device)

    def __len__(self):
        return self.sizes.shape[0]

    def require_window(self, img_size: int):
        """Every image must hold the (2 S) x (3 S) window the crop keeps (torchvision's crops raise or pad otherwise)."""
        small = ((self.sizes[:, 0] < 2 * img_size) | (self.sizes[:, 1] < 3 * img_size)).nonzero().flatten().tolist()
        if small:
            k = small[0]
            raise ValueError(f'{len(small)} image(s) are smaller than the {2 * img_size} x {3 * img_size} crop window, the first is '
                             f'image {k} with {int(self.sizes[k, 0])} x {int(self.sizes[k, 1])}')


def _plan_inputs(u: torch.Tensor, image: torch.Tensor, sizes: torch.Tensor):
    """What every ``*_augment_plan`` starts from: (u as fp64, the image indices as int64 on u's device, H, W fp64 [B] of those
    images - looked up with the index clamped into the table; the index itself is returned as given - and zeros, ones like H)."""
    u = u.double()
    image = image.to(device=u.device, dtype=torch.int64)
    hw = sizes.to(u.device)[image.clamp(0, sizes.shape[0] - 1)]
    H, W = hw[:, 0].double(), hw[:, 1].double()
    return u, image, H, W, torch.zeros_like(H), torch.ones_like(H)


def _inclusive_draw(t: torch.Tensor, lo, hi):
    """random.randint(lo, hi) from uniforms ``t``: lo + floor(t (hi - lo + 1)), never above hi; lo / hi numbers or tensors like t."""
    span = torch.as_tensor(hi - lo, dtype=t.dtype, device=t.device)
    return torch.minimum(torch.floor(t * (span + 1)), span) + lo


def _padded_crop_origin(t: torch.Tensor, size: torch.Tensor, S: int):
    """RandomCrop(S, pad_if_needed=True) along one axis of ``size`` pixels: a draw in [0, size + 2 pad - S] less pad = max(S - size, 0)."""
    pad = (S - size).clamp_(min=0)
    return _inclusive_draw(t, 0.0, size + 2 * pad - S) - pad


def _inverse_shift_scale_rotate(u: torch.Tensor, warp: torch.Tensor, angle, scale, H, W, ident):
    """A.ShiftScaleRotate from ``u`` fp64 [B, 4]: angle = u a - b degrees for (a, b) = ``angle``, scale = u a + b for ``scale``, dx, dy
    ~ U(-0.05, 0.05) of W, H.  fp64 [B, 6]: where ``warp``, the inverse of  getRotationMatrix2D((W / 2 - 0.5, H / 2 - 0.5), angle,
    scale) + (dx, dy), inverted as cv2.warpAffine does without WARP_INVERSE_MAP; elsewhere ``ident``."""
    angle, scale = (u[:, 0] * angle[0] - angle[1]) * (torch.pi / 180.0), u[:, 1] * scale[0] + scale[1]
    dx, dy = (u[:, 2] * 0.1 - 0.05) * W, (u[:, 3] * 0.1 - 0.05) * H
    cx, cy = W / 2 - 0.5, H / 2 - 0.5
    alpha, beta = torch.cos(angle) * scale, torch.sin(angle) * scale
    m0, m1, m2 = alpha, beta, (1 - alpha) * cx - beta * cy + dx            # cv2.getRotationMatrix2D, then the translation
    m3, m4, m5 = -beta, alpha, beta * cx + (1 - alpha) * cy + dy
    det = m0 * m4 - m1 * m3
    d = torch.where(det != 0, 1.0 / det, torch.zeros_like(det))
    i0, i1, i3, i4 = m4 * d, m1 * (-d), m3 * (-d), m0 * d
    i2, i5 = -(i0 * m2) - i1 * m5, -(i3 * m2) - i4 * m5
    return torch.where(warp.unsqueeze(1), torch.stack([i0, i1, i2, i3, i4, i5], dim=1), ident)


def _jitter_draws(u: torch.Tensor, jitter: torch.Tensor, factor_ranges, hue_range):
    """ColorJitter's draws from ``u`` fp64 [B, 8] (four order keys, brightness, contrast, saturation, hue) where ``jitter``:
    (order int32 [B, 4], the stable argsort of the keys; factors fp32 [B, 3], u a + b per (a, b) of ``factor_ranges``; hue int32 [B],
    the uint8 shift trunc((u a - b) 255) mod 256 for (a, b) = ``hue_range``); elsewhere the natural order, factors 1, shift 0."""
    natural = torch.arange(4, dtype=torch.int32, device=u.device).expand(u.shape[0], 4)
    order = torch.where(jitter.unsqueeze(1), torch.argsort(u[:, 0:4], dim=1, stable=True).to(torch.int32), natural)
    drawn = torch.stack([u[:, 4 + k] * a + b for k, (a, b) in enumerate(factor_ranges)], dim=1)
    factors = torch.where(jitter.unsqueeze(1), drawn, torch.ones_like(drawn)).float()
    hue = torch.where(jitter, torch.trunc((u[:, 7] * hue_range[0] - hue_range[1]) * 255.0).to(torch.int64) % 256, 0).to(torch.int32)
    return order, factors, hue


def div2k_augment_plan(u: torch.Tensor, image: torch.Tensor, sizes: torch.Tensor, img_size: int, train: bool = True):
    """The random choices of ``DIV2KPatch.read_image`` and of the crop of ``__getitem__`` (div2k_patch.py:89-111) for a whole batch at
    once, from uniform numbers ``u`` [B, 13] in [0, 1) (columns: horizontal flip, vertical flip, warp, angle, scale, dx, dy, colour
    shift, its three channel shifts, crop top, crop left), the image indices ``image`` [B] and ``sizes`` int32 [n, 2] = (H, W):
      image int32 [B]      the indices
      flags int32 [B]      bit 0 / 1: RandomHorizontalFlip / RandomVerticalFlip (p = 0.5); bit 2: A.ShiftScaleRotate (p = 0.5);
                           bit 3: A.RGBShift (p = 0.5)
      minv  fp64  [B, 6]   inverse of  getRotationMatrix2D((W / 2 - 0.5, H / 2 - 0.5), angle ~ U(-20, 20), scale ~ U(0.85, 1.15))
                           + (dx W, dy H), dx, dy ~ U(-0.05, 0.05), inverted as cv2.warpAffine does; the identity with the warp off
      rgb   fp32  [B, 3]   channel shifts ~ U(-15, 15); 0 with the colour shift off
      crop  int32 [B, 2]   RandomCrop origin floor(u (H - 2 S + 1)), floor(u (W - 3 S + 1))
    ``train=False``: no augmentation and CenterCrop's origin int(round((H - 2 S) / 2)) (round half to even).  Elementwise torch
    operations on the device of ``u``: no host copy, no sync; every fp64 product and sum is an operation of its own."""
    u, image, H, W, zero, one = _plan_inputs(u, image, sizes)
    n_rows = u.shape[0]
    room_y, room_x = (H - 2 * img_size).clamp_(min=0), (W - 3 * img_size).clamp_(min=0)
    minv = torch.stack([one, zero, zero, zero, one, zero], dim=1)
    if not train:
        flags = torch.zeros(n_rows, dtype=torch.int32, device=u.device)
        rgb = torch.zeros(n_rows, 3, dtype=torch.float32, device=u.device)
        crop = torch.stack([torch.round(room_y / 2), torch.round(room_x / 2)], dim=1).to(torch.int32)
        return image.to(torch.int32), flags, minv.contiguous(), rgb, crop.contiguous()
    hflip, vflip, warp, colour = u[:, 0] < 0.5, u[:, 1] < 0.5, u[:, 2] < 0.5, u[:, 7] < 0.5
    flags = (hflip.int() + 2 * vflip.int() + 4 * warp.int() + 8 * colour.int()).to(torch.int32)
    minv = _inverse_shift_scale_rotate(u[:, 3:7], warp, (40.0, 20.0), (0.3, 0.85), H, W, minv)
    rgb = ((u[:, 8:11] * 30.0 - 15.0) * colour.unsqueeze(1)).float()
    crop = torch.stack([_inclusive_draw(u[:, 11], 0.0, room_y), _inclusive_draw(u[:, 12], 0.0, room_x)], dim=1).to(torch.int32)   # no padding
    return image.to(torch.int32), flags, minv.contiguous(), rgb.contiguous(), crop.contiguous()


class _DeviceLoader:
    """What the device loaders share: ``store`` holds the images, an epoch is ``len(store) * repeat`` samples dealt to ``world``
    ranks in whole batches, and every random stream of an epoch is seeded from (seed, epoch, stream number)."""

    def __init__(self, store: Div2kImageStore, batch_size: int, repeat: int, rank: int, world: int, seed: int):
        if not 0 <= rank < world:
            raise ValueError(f'rank {rank} outside a world of {world}')
        self.store, self.batch_size, self.repeat, self.rank, self.world, self.seed = store, int(batch_size), int(repeat), rank, world, seed
        self.epoch = 0
        if len(self) < 1:
            raise ValueError(f'{len(store)} images x {repeat} over {world} rank(s) do not fill one batch of {batch_size}')

    def set_epoch(self, epoch: int):
        self.epoch = int(epoch)

    def __len__(self):
        return len(self.store) * self.repeat // self.world // self.batch_size

    def _generator(self, stream: int):
        g = torch.Generator(device=self.store.device)
        g.manual_seed((self.seed * 1000003 + self.epoch) * 4099 + stream)
        return g


class Div2kDeviceLoader(_DeviceLoader):
    """The DIV2K pair loader on the device: what ``build_loader`` + ``DIV2KPatch`` + ``DevicePrefetcher`` deliver, from a
    ``Div2kImageStore``, without a host copy or a sync per batch.  An epoch is a permutation (drawn on the device, the same on
    every rank) of the image indices repeated ``repeat`` times, of which rank r takes every ``world``-th from r on; the last
    incomplete batch is dropped.  Each batch: uniforms -> ``div2k_augment_plan`` -> ``ops.div2k_regions_u8`` -> ``div2k_pair_plan``
    -> ``assemble_pairs``; it yields (pairs uint8 [B, 2, 3, S, S], labels fp32 [B, 4]) for ``TrainStep.step``."""

    def __init__(self, store: Div2kImageStore, batch_size: int, img_size: int, erosion_ratio: float, with_negative: bool = True,
                 train: bool = True, repeat: int = 5, rank: int = 0, world: int = 1, seed: int = 0):
        store.require_window(img_size)
        super().__init__(store, batch_size, repeat, rank, world, seed)
        self.img_size, self.erosion_ratio, self.with_negative, self.train = int(img_size), float(erosion_ratio), with_negative, train

    def epoch_order(self) -> torch.Tensor:
        """The epoch's permutation of the repeated image indices (int64 on the store's device), before sharding."""
        n = len(self.store)
        return torch.randperm(n * self.repeat, generator=self._generator(0), device=self.store.device) % n

    def rank_indices(self) -> torch.Tensor:
        """[len(self), batch_size]: the image index of every sample this rank sees in the epoch."""
        per_rank = len(self.store) * self.repeat // self.world
        mine = self.epoch_order()[self.rank::self.world][:per_rank]
        return mine[: len(self) * self.batch_size].view(len(self), self.batch_size)

    def plan(self, image: torch.Tensor, generator: torch.Generator):
        """One batch's draws: (the five tensors of ``div2k_augment_plan``, the three of ``div2k_pair_plan``)."""
        u = torch.rand(image.numel(), 17, generator=generator, device=self.store.device)
        return (div2k_augment_plan(u[:, :13], image, self.store.sizes_dev, self.img_size, self.train),
                div2k_pair_plan(u[:, 13:], self.img_size, self.erosion_ratio, self.with_negative, self.train))

    def __iter__(self):
        g = self._generator(1 + self.rank)
        for image in self.rank_indices():
            (idx, flags, minv, rgb, crop), (cells, labels, erode) = self.plan(image, g)
            regions = ops.div2k_regions_u8(self.store.data, self.store.offsets_dev, self.store.sizes_dev, idx, flags, minv, rgb, crop,
                                           self.img_size)
            yield assemble_pairs(regions, cells, erode, self.img_size), labels


# ---- config H's input pipeline on the device (hisfrag.py:63-115)
HISFRAG_PLAN_COLUMNS = 21


class HisfragPlan(NamedTuple):
    """One batch's per-sample arguments of ``ops.hisfrag_windows_u8`` / ``hisfrag_jitter_u8`` / ``hisfrag_blur_u8``."""
    image: torch.Tensor      # int32 [B]     image index
    flags: torch.Tensor      # int32 [B]     bit 0 RandomAffine, bit 1 ShiftScaleRotate, bit 2 ColorJitter, bit 3 GaussianBlur
    afix: torch.Tensor       # int64 [B, 6]  Pillow's 16.16 coefficients a0..a5 of the RandomAffine matrix
    minv: torch.Tensor       # fp64  [B, 6]  inverse ShiftScaleRotate matrix
    origin: torch.Tensor     # int32 [B, 2]  (top, left) of the window in unpadded image coordinates
    order: torch.Tensor      # int32 [B, 4]  jitter operations in the order they run (0 brightness, 1 contrast, 2 saturation, 3 hue)
    factors: torch.Tensor    # fp32  [B, 3]  brightness, contrast, saturation factors
    hue: torch.Tensor        # int32 [B]     the uint8 added to H
    blur: torch.Tensor       # fp32  [B, 2]  (k_edge, k_mid) of the 3-tap Gaussian


def hisfrag_augment_plan(u: torch.Tensor, image: torch.Tensor, sizes: torch.Tensor, img_size: int, train: bool = True) -> HisfragPlan:
    """The random choices of ``HisfragTrainer.get_transforms`` (hisfrag.py:66-78) for a whole batch at once, from uniform numbers
    ``u`` [B, 21] in [0, 1), the image indices ``image`` [B] and ``sizes`` int32 [n, 2] = (H, W).  Columns of ``u``:
      0-2    RandomAffine(5, translate=(0.1, 0.1)): angle ~ U(-5, 5), tx = round(U(-0.1 W, 0.1 W)), ty likewise (half to even);
             the matrix is torchvision's _get_inverse_affine_matrix about (0.5 W, 0.5 H), its 16.16 form Pillow's FIX
      3-7    A.ShiftScaleRotate at p = 0.5: angle ~ U(-10, 10), scale ~ U(0.9, 1.1), dx, dy ~ U(-0.05, 0.05) of W, H; the forward
             matrix and its inversion as in ``div2k_augment_plan``
      8-9    RandomCrop(S, pad_if_needed=True): origin floor(u (Hp - S + 1)) - pad, pad = max(S - H, 0), Hp = H + 2 pad
      10-18  ColorJitter(0.3, 0.3, 0.3, 0.3) at p = 0.5: the order is the argsort of four uniforms, brightness / contrast /
             saturation ~ U(0.7, 1.3), hue ~ U(-0.3, 0.3) as the uint8 shift trunc(hue 255) mod 256
      19-20  GaussianBlur((3, 3), (1, 2)) at p = 0.5: sigma ~ U(1, 2), e = exp(-0.5 / sigma^2) rounded to fp32 once, then
             k_edge = e / (e + 1 + e), k_mid = 1 / (e + 1 + e) in fp32
    ``train=False``: everything off and CenterCrop's origin (round half to even; torchvision's centre padding for an image smaller
    than S).  Elementwise torch operations on the device of ``u``: no host copy, no sync; fp64 throughout, every product and sum
    an operation of its own."""
    u, image, H, W, zero, one = _plan_inputs(u, image, sizes)
    n_rows, dev, S = u.shape[0], u.device, int(img_size)
    ident = torch.stack([one, zero, zero, zero, one, zero], dim=1)
    ident_fix = torch.tensor([65536, 0, 32768, 0, 65536, 32768], dtype=torch.int64, device=dev).expand(n_rows, 6)
    natural = torch.arange(4, dtype=torch.int32, device=dev).expand(n_rows, 4)
    no_blur = torch.tensor([0.0, 1.0], dtype=torch.float32, device=dev).expand(n_rows, 2)
    if not train:
        # on purpose not ``michigan_augment_plan``'s ``centre``: CenterCrop pads a deficit d by d // 2 in front, PadCenterCrop by d and re-crops
        centre = lambda n: torch.where(n >= S, torch.round((n - S) / 2), -torch.floor((S - n) / 2))
        return HisfragPlan(image.to(torch.int32), torch.zeros(n_rows, dtype=torch.int32, device=dev), ident_fix.contiguous(), ident.contiguous(),
                           torch.stack([centre(H), centre(W)], dim=1).to(torch.int32).contiguous(), natural.contiguous(),
                           torch.ones(n_rows, 3, dtype=torch.float32, device=dev), torch.zeros(n_rows, dtype=torch.int32, device=dev),
                           no_blur.contiguous())
    warp, jitter, blur_on = u[:, 3] < 0.5, u[:, 10] < 0.5, u[:, 19] < 0.5
    flags = (1 + 2 * warp.int() + 4 * jitter.int() + 8 * blur_on.int()).to(torch.int32)
    # RandomAffine
    rot = (u[:, 0] * 10.0 - 5.0) * (torch.pi / 180.0)
    tx, ty = torch.round((u[:, 1] * 2.0 - 1.0) * (0.1 * W)), torch.round((u[:, 2] * 2.0 - 1.0) * (0.1 * H))
    cx, cy = W * 0.5, H * 0.5
    cos, sin = torch.cos(rot), torch.sin(rot)
    M0, M1, M3, M4 = cos, sin, -sin, cos
    M2 = (M0 * (-cx - tx) + M1 * (-cy - ty)) + cx
    M5 = (M3 * (-cx - tx) + M4 * (-cy - ty)) + cy
    fix = lambda t: torch.floor(t * 65536.0 + 0.5).to(torch.int64)
    afix = torch.stack([fix(M0), fix(M1), fix(M2 + M0 * 0.5 + M1 * 0.5), fix(M3), fix(M4), fix(M5 + M3 * 0.5 + M4 * 0.5)], dim=1)
    # ShiftScaleRotate
    minv = _inverse_shift_scale_rotate(u[:, 4:8], warp, (20.0, 10.0), (0.2, 0.9), H, W, ident)
    # RandomCrop with pad_if_needed
    origin = torch.stack([_padded_crop_origin(u[:, 8], H, S), _padded_crop_origin(u[:, 9], W, S)], dim=1).to(torch.int32)
    # ColorJitter
    order, factors, hue = _jitter_draws(u[:, 11:19], jitter, ((0.6, 0.7), (0.6, 0.7), (0.6, 0.7)), (0.6, 0.3))
    # GaussianBlur
    inv_sigma = 1.0 / (u[:, 20] + 1.0)
    e = torch.exp(-0.5 * (inv_sigma * inv_sigma)).float()
    den = (e + 1.0) + e
    blur = torch.where(blur_on.unsqueeze(1), torch.stack([e / den, 1.0 / den], dim=1), no_blur)
    return HisfragPlan(image.to(torch.int32), flags, afix.contiguous(), minv.contiguous(), origin.contiguous(), order.contiguous(),
                       factors.contiguous(), hue.contiguous(), blur.contiguous())


def hisfrag_feed(store: 'Div2kImageStore', plan: HisfragPlan, img_size: int) -> torch.Tensor:
    """``plan`` -> uint8 [B, 3, S, S] on the store's device: geometry, colour jitter and blur, three entry points back to back."""
    windows = ops.hisfrag_windows_u8(store.data, store.offsets_dev, store.sizes_dev, plan.image, plan.flags, plan.afix, plan.minv,
                                     plan.origin, img_size)
    jittered = ops.hisfrag_jitter_u8(windows, plan.flags, plan.order, plan.factors, plan.hue, out=windows)     # pointwise: in place
    return ops.hisfrag_blur_u8(jittered, plan.flags, plan.blur)


class HisfragDeviceLoader(_DeviceLoader):
    """Config H's training loader on the device: what ``HisfragTrainer.get_dataloader`` (hisfrag.py:101-115) delivers, from a
    ``Div2kImageStore`` of the decoded fragments and their writer ids ``labels``, without a host copy or a sync per batch.
    Sampling is ``MPerClassSampler(labels, m)``'s scheme: passes over a device-drawn permutation of the writers, ``m`` members
    per writer (a random order without repetition where the writer has at least ``m``, cycling through a random order of its
    members where it has fewer), passes concatenated and cut into batches.  Every rank draws from its own generator stream (the
    reference's sampler is not distributed either).  Each batch: uniforms -> ``hisfrag_augment_plan`` -> ``hisfrag_feed``; it yields
    (images uint8 [B, 3, S, S], targets int64 [B]) for ``hisfrag_prepare_data``.  Images smaller than the window are padded."""
    plan_columns, augment_plan, feed = HISFRAG_PLAN_COLUMNS, staticmethod(hisfrag_augment_plan), staticmethod(hisfrag_feed)   # a subclass: its own

    def __init__(self, store: Div2kImageStore, labels, batch_size: int, img_size: int, m: int = 3, train: bool = True, repeat: int = 1,
                 rank: int = 0, world: int = 1, seed: int = 0):
        super().__init__(store, batch_size, repeat, rank, world, seed)
        labels = torch.as_tensor(labels).reshape(-1).to(torch.int64).cpu()
        if labels.numel() != len(store):
            raise ValueError(f'{labels.numel()} labels for {len(store)} images')
        if m < 1 or batch_size % m:
            raise ValueError(f'batch size {batch_size} is no multiple of m = {m}')
        self.img_size, self.m, self.train = int(img_size), int(m), train
        writers, member_of = torch.unique(labels, return_inverse=True)
        counts = torch.bincount(member_of, minlength=writers.numel())
        table = torch.zeros(writers.numel(), int(counts.max()), dtype=torch.int64)      # the writers' members, padded with 0
        for w in range(writers.numel()):
            table[w, : int(counts[w])] = (member_of == w).nonzero().flatten()
        dev = store.device
        self.labels_dev, self.members_dev, self.counts_dev = labels.to(dev), table.to(dev), counts.to(dev)

    def rank_indices(self) -> torch.Tensor:
        """[len(self), batch_size]: the image index of every sample this rank sees in the epoch (int64 on the store's device)."""
        dev, m = self.store.device, self.m
        n_writers, width = self.members_dev.shape
        need = len(self) * self.batch_size
        passes = -(-need // (n_writers * m))
        g = self._generator(2 * self.rank)
        writer = torch.stack([torch.randperm(n_writers, generator=g, device=dev) for _ in range(passes)])            # [passes, writers]
        keys = torch.rand(passes, n_writers, width, generator=g, device=dev)
        count = self.counts_dev[writer]                                                                              # [passes, writers]
        keys = torch.where(torch.arange(width, device=dev) < count.unsqueeze(2), keys, 2.0)                          # padding sorts last
        shuffled = torch.argsort(keys, dim=2)                                                # the real members first, in a random order
        take = torch.arange(m, device=dev).expand(passes, n_writers, m) % count.unsqueeze(2)
        picked = self.members_dev[writer.unsqueeze(2), shuffled.gather(2, take)]                                     # [passes, writers, m]
        return picked.reshape(-1)[:need].view(len(self), self.batch_size)

    def plan(self, image: torch.Tensor, generator: torch.Generator):
        """One batch's draws (a ``HisfragPlan``; whatever ``augment_plan`` returns in a subclass)."""
        u = torch.rand(image.numel(), self.plan_columns, generator=generator, device=self.store.device)
        return self.augment_plan(u, image, self.store.sizes_dev, self.img_size, self.train)

    def __iter__(self):
        g = self._generator(2 * self.rank + 1)
        for image in self.rank_indices():
            yield self.feed(self.store, self.plan(image, g), self.img_size), self.labels_dev[image]


# ---- michigan.py's input pipeline on the device (michigan.py:68-101)
MICHIGAN_PLAN_COLUMNS = 104
MICHIGAN_MAX_HOLES = 16
_RRC_ATTEMPTS = 10


class MichiganPlan(NamedTuple):
    """One batch's per-sample arguments of ``ops.michigan_windows_u8`` / ``hisfrag_jitter_u8`` / ``michigan_blur_gray_u8``."""
    image: torch.Tensor      # int32 [B]         image index
    flags: torch.Tensor      # int32 [B]         bit 0 dropout, 1 horizontal flip, 2 ColorJitter, 3 GaussianBlur, 4 vertical flip, 5 grey
    origin: torch.Tensor     # int32 [B, 2]      (top, left) of the window in unpadded image coordinates
    box: torch.Tensor        # int32 [B, 4]      RandomResizedCrop's (i, j, h, w) in the window (what the tap tables were made from)
    x0: torch.Tensor         # int32 [B, S]      first horizontal tap per output column, in window coordinates
    kx: torch.Tensor         # int32 [B, S, 3]   its 22-bit fixed-point weights
    y0: torch.Tensor         # int32 [B, S]      first vertical tap per output row
    ky: torch.Tensor         # int32 [B, S, 3]
    holes: torch.Tensor      # int32 [B, 16, 4]  (x1, y1, x2, y2), half-open, before the flips
    n_holes: torch.Tensor    # int32 [B]
    order: torch.Tensor      # int32 [B, 4]      jitter operations in the order they run (0 brightness, 1 contrast, 2 saturation, 3 hue)
    factors: torch.Tensor    # fp32  [B, 3]      brightness, contrast, saturation factors
    hue: torch.Tensor        # int32 [B]         the uint8 added to H
    blur: torch.Tensor       # int32 [B, 2]      (ww, fw) of Pillow's box blur


def _bilinear_taps(in_size: torch.Tensor, out_size: int, first: torch.Tensor, index: torch.Tensor):
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc for the bilinear filter where it scales up (support 1, three taps): per
    sample ``in_size`` fp64 [B] source pixels starting at ``first`` fp64 [B] are resized to ``out_size``; for the output indices
    ``index`` fp64 [n] -> (first tap int32 [B, n], weights int32 [B, n, 3])."""
    scale = in_size / torch.full_like(in_size, float(out_size))          # a tensor divisor: a true division on every device
    center = (index.unsqueeze(0) + 0.5) * scale.unsqueeze(1)
    xmin = torch.trunc(center - 1.0 + 0.5).clamp_(min=0)
    xmax = torch.minimum(torch.trunc(center + 1.0 + 0.5), in_size.unsqueeze(1)) - xmin
    w = []
    for t in range(3):
        wt = (1.0 - torch.abs((t + xmin) - center + 0.5)).clamp_(min=0)
        w.append(torch.where(t < xmax, wt, torch.zeros_like(wt)))
    ww = (w[0] + w[1]) + w[2]
    k = torch.stack([torch.trunc(0.5 + (wt / ww) * float(1 << 22)) for wt in w], dim=2)
    return (xmin + first.unsqueeze(1)).to(torch.int32).contiguous(), k.to(torch.int32).contiguous()


def michigan_augment_plan(u: torch.Tensor, image: torch.Tensor, sizes: torch.Tensor, img_size: int, train: bool = True,
                          holes=(3, 16), hole_size=(16, 64), radius_max: float = 1.0) -> MichiganPlan:
    """The random choices of michigan.py's ``HisfragTrainer.get_transforms`` (michigan.py:71-85) for a whole batch at once, from
    uniform numbers ``u`` [B, 104] in [0, 1), the image indices ``image`` [B] and ``sizes`` int32 [n, 2] = (H, W).  Columns of ``u``:
      0-1      RandomCrop(S, pad_if_needed=True, fill 255): origin floor(u (Hp - S + 1)) - pad, pad = max(S - H, 0), Hp = H + 2 pad
      2-21     RandomResizedCrop(S, scale=(0.6, 1)) on the window: ten attempts of (area, ratio) uniforms, area = (0.6 + 0.4 u) S^2,
               ratio = exp(log(3/4) + u (log(4/3) - log(3/4))), w = round(sqrt(area ratio)), h = round(sqrt(area / ratio)) (half to
               even); the first attempt with 0 < w <= S and 0 < h <= S wins, otherwise the whole window
      22-23    its position: i = floor(u (S - h + 1)), j = floor(u (S - w + 1)); the tap tables are Pillow's bilinear coefficients for
               (h, w) -> (S, S), first taps offset by (i, j)
      24-25    CoarseDropout at p = 0.9; the number of holes, an inclusive integer draw lo + floor(u (hi - lo + 1)) in ``holes``
      26-89    per hole (height, width, y1, x1): height / width inclusive draws in ``hole_size`` clamped to S, y1 in [0, S - height],
               x1 in [0, S - width]
      90-91    horizontal, vertical flip at p = 0.5
      92-100   ColorJitter(0.2, 0.3, 0.3, 0.1) at p = 0.5: the order is the argsort of four uniforms, brightness ~ U(0.8, 1.2),
               contrast / saturation ~ U(0.7, 1.3), hue ~ U(-0.1, 0.1) as the uint8 shift trunc(hue 255) mod 256
      101-102  GaussianBlur at p = 0.5: r = fp32(0.1 + (radius_max - 0.1) u), then in fp32 s = r r / 3, a = (-(3 s)) / (6 (s - 1)),
               ww = trunc(2^24 / (a 2 + 1)), and fw = (2^24 - ww) // 2 (Pillow's box radius is 0 for every r <= 1)
      103      RandomGrayscale at p = 0.2
    ``train=False``: PadCenterCrop((S, S), fill 255) -> Resize(R = int(1.15 S)) -> CenterCrop(S): the origin is round((W - S) / 2) for
    W >= S and round(d / 2) - d for a deficit d = S - W (the reference pads both sides by d), the tables are those of S -> R at the
    output indices x + round((R - S) / 2), every flag is 0.  Elementwise torch operations on the device of ``u``: no host copy, no
    sync; fp64 except where stated, every product and sum an operation of its own."""
    S = int(img_size)
    lo_n, hi_n = (int(t) for t in holes)
    lo_s, hi_s = (int(t) for t in hole_size)
    if not 0 <= lo_n <= hi_n <= MICHIGAN_MAX_HOLES or not 1 <= lo_s <= hi_s:
        raise ValueError(f'holes {holes} must lie in 0..{MICHIGAN_MAX_HOLES} and hole_size {hole_size} be positive, both ascending')
    if not 0.1 <= radius_max <= 1.0:
        raise ValueError(f'radius_max {radius_max} outside [0.1, 1]: beyond 1 Pillow\'s box radius is no longer 0')
    u, image, H, W, zero, one = _plan_inputs(u, image, sizes)
    n_rows, dev = u.shape[0], u.device
    izero = torch.zeros(n_rows, dtype=torch.int32, device=dev)
    natural = torch.arange(4, dtype=torch.int32, device=dev).expand(n_rows, 4)
    no_blur = torch.tensor([1 << 24, 0], dtype=torch.int32, device=dev).expand(n_rows, 2)
    no_holes = torch.zeros(n_rows, MICHIGAN_MAX_HOLES, 4, dtype=torch.int32, device=dev)
    index = torch.arange(S, dtype=torch.float64, device=dev)
    full = one * S
    if not train:
        centre = lambda n: torch.where(n >= S, torch.round((n - S) / 2), torch.round((S - n) / 2) - (S - n))
        R = int(S * 1.15)
        x0, kx = _bilinear_taps(full, R, zero, index + round((R - S) / 2))
        box = torch.stack([zero, zero, full, full], dim=1).to(torch.int32)
        return MichiganPlan(image.to(torch.int32), izero, torch.stack([centre(H), centre(W)], dim=1).to(torch.int32).contiguous(),
                            box.contiguous(), x0, kx, x0.clone(), kx.clone(), no_holes, izero.clone(), natural.contiguous(),
                            torch.ones(n_rows, 3, dtype=torch.float32, device=dev), izero.clone(), no_blur.contiguous())
    draw = _inclusive_draw
    # RandomCrop with pad_if_needed
    origin = torch.stack([_padded_crop_origin(u[:, 0], H, S), _padded_crop_origin(u[:, 1], W, S)], dim=1).to(torch.int32)
    # RandomResizedCrop
    log_lo, log_hi = math.log(3.0 / 4.0), math.log(4.0 / 3.0)
    area = (u[:, 2:22:2] * 0.4 + 0.6) * float(S * S)
    ratio = torch.exp(u[:, 3:22:2] * (log_hi - log_lo) + log_lo)
    w_try, h_try = torch.round(torch.sqrt(area * ratio)), torch.round(torch.sqrt(area / ratio))
    valid = (w_try > 0) & (w_try <= S) & (h_try > 0) & (h_try <= S)
    first = (valid.int().cumsum(1) == 0).sum(1)                            # the attempts in front of the first valid one
    pick = first.clamp(max=_RRC_ATTEMPTS - 1).unsqueeze(1)
    found = first < _RRC_ATTEMPTS
    bw, bh = torch.where(found, w_try.gather(1, pick).squeeze(1), full), torch.where(found, h_try.gather(1, pick).squeeze(1), full)
    bi, bj = torch.where(found, draw(u[:, 22], 0.0, S - bh), zero), torch.where(found, draw(u[:, 23], 0.0, S - bw), zero)
    x0, kx = _bilinear_taps(bw, S, bj, index)
    y0, ky = _bilinear_taps(bh, S, bi, index)
    # CoarseDropout
    dropout = u[:, 24] < 0.9
    count = torch.where(dropout, draw(u[:, 25], float(lo_n), float(hi_n)), zero)
    hu = u[:, 26:90].reshape(n_rows, MICHIGAN_MAX_HOLES, 4)
    limit = lambda t: t.clamp(max=float(S))
    hh = limit(draw(hu[:, :, 0], float(lo_s), float(hi_s)))
    hwid = limit(draw(hu[:, :, 1], float(lo_s), float(hi_s)))
    y1, x1 = draw(hu[:, :, 2], 0.0, S - hh), draw(hu[:, :, 3], 0.0, S - hwid)
    used = torch.arange(MICHIGAN_MAX_HOLES, device=dev).unsqueeze(0) < count.unsqueeze(1)
    rects = torch.where(used.unsqueeze(2), torch.stack([x1, y1, x1 + hwid, y1 + hh], dim=2), zero.view(-1, 1, 1)).to(torch.int32)
    # flips, jitter, blur, grey
    hflip, vflip, jitter, blur_on, grey = u[:, 90] < 0.5, u[:, 91] < 0.5, u[:, 92] < 0.5, u[:, 101] < 0.5, u[:, 103] < 0.2
    flags = (dropout.int() + 2 * hflip.int() + 4 * jitter.int() + 8 * blur_on.int() + 16 * vflip.int() + 32 * grey.int()).to(torch.int32)
    order, factors, hue = _jitter_draws(u[:, 93:101], jitter, ((0.4, 0.8), (0.6, 0.7), (0.6, 0.7)), (0.2, 0.1))
    r = (u[:, 102] * (float(radius_max) - 0.1) + 0.1).float()              # Pillow takes the radius as a C float: fp32 from here on
    s2 = (r * r) / torch.full_like(r, 3.0)                                  # tensor divisors: true divisions on every device
    a = (-(s2 * 3.0)) / ((s2 - 1.0) * 6.0)
    ww = torch.trunc(16777216.0 / (a * 2.0 + 1.0)).to(torch.int64)
    fw = torch.div((1 << 24) - ww, 2, rounding_mode='floor')
    blur = torch.where(blur_on.unsqueeze(1), torch.stack([ww, fw], dim=1).to(torch.int32), no_blur)
    box = torch.stack([bi, bj, bh, bw], dim=1).to(torch.int32)
    return MichiganPlan(image.to(torch.int32), flags, origin.contiguous(), box.contiguous(), x0, kx, y0, ky, rects.contiguous(),
                        count.to(torch.int32), order.contiguous(), factors.contiguous(), hue.contiguous(), blur.contiguous())


def michigan_feed(store: 'Div2kImageStore', plan: MichiganPlan, img_size: int) -> torch.Tensor:
    """``plan`` -> uint8 [B, 3, S, S] on the store's device: geometry, colour jitter, blur and grey, three entry points back to back."""
    windows = ops.michigan_windows_u8(store.data, store.offsets_dev, store.sizes_dev, plan.image, plan.flags, plan.origin, plan.x0,
                                      plan.kx, plan.y0, plan.ky, plan.holes, plan.n_holes, img_size)
    jittered = ops.hisfrag_jitter_u8(windows, plan.flags, plan.order, plan.factors, plan.hue, out=windows)     # pointwise: in place
    return ops.michigan_blur_gray_u8(jittered, plan.flags, plan.blur)


class MichiganDeviceLoader(HisfragDeviceLoader):
    """michigan.py's training loader on the device: ``HisfragDeviceLoader``'s sampler, epochs, ranks and generator streams, with
    michigan.py's transforms (michigan.py:68-101).  Each batch: uniforms -> ``michigan_augment_plan`` -> ``michigan_feed``; it yields
    (images uint8 [B, 3, S, S], targets int64 [B]) for ``hisfrag_prepare_data``.  Images smaller than the window are padded with
    255.  The reference runs 20 passes over the set per epoch (michigan.py:110-112): that is the caller's ``repeat``."""
    plan_columns, augment_plan, feed = MICHIGAN_PLAN_COLUMNS, staticmethod(michigan_augment_plan), staticmethod(michigan_feed)


# ---- Pillow-exact resize from the store: the Pajigsaw loader and the evaluation feeds (pajigsaw.py, michigan.py:90-96,
# hisfrag.py:163-211)
def _half(n: int) -> int:
    """torchvision's crop origin int(round(n / 2.0)): Python's round, half to even."""
    return int(round(n / 2.0))


def _square_tables(store: Div2kImageStore, size: int):
    """``ops.resample_tables`` of the sides of the store's square images -> ``size``, made once per (store, size)."""
    cache = store.__dict__.setdefault('_square_tables', {})
    if size not in cache:
        square = store.sizes[store.sizes[:, 0] == store.sizes[:, 1]]
        if square.shape[0] == 0:
            raise ValueError(f'resize_images: none of the {len(store)} stored images is square')
        cache[size] = ops.resample_tables(square[:, 0].tolist(), size, store.device)
    return cache[size]


def _require_square(store: Div2kImageStore, image, size: int, names=None):
    """Resize(S) takes the shorter side to S and keeps the aspect ratio; the model takes S x S only.  ``image``: the indices that
    will be read where the host knows them (a list or a CPU tensor), else None: then every stored image must be square."""
    sizes = store.sizes if image is None else store.sizes[torch.as_tensor(image, dtype=torch.int64).reshape(-1).clamp(0, len(store) - 1)]
    bad = (sizes[:, 0] != sizes[:, 1]).nonzero().flatten().tolist()
    if bad:
        k = bad[0] if image is None else int(torch.as_tensor(image).reshape(-1)[bad[0]])
        name = f'image {k}' if names is None else f'{names[k]!r} (image {k})'
        raise ValueError(f'{name} is {int(store.sizes[k, 0])} x {int(store.sizes[k, 1])}: Resize({size}) keeps its aspect ratio, and the model '
                         f'takes square {size} x {size} images only ({len(bad)} such image(s))')


def resize_images(store: Div2kImageStore, image, img_size: int, out: torch.Tensor | None = None) -> torch.Tensor:
    """``TwoImgSyncEval.normalize``'s ``Resize(img_size)`` (data/transforms.py:14-18) of the stored images ``image`` (indices [n]: a
    list, or an integer tensor on any device) -> uint8 [n, 3, S, S] on the store's device, Pillow's 8-bit bilinear resize bit for
    bit at any scale up to 8x down (``ops.resample_u8``); ToTensor + Normalize are folded into the patch-embedding kernel.  The
    shorter side goes to S, so a square image gives S x S; a non-square one is refused by name (indices that live on the device are
    not read back: then every stored image must be square).  ``out``: a destination view,
    ``pairs[:, 0]`` of a [B, 2, 3, S, S] tensor for one."""
    S = int(img_size)
    on_host = not torch.is_tensor(image) or not image.is_cuda
    _require_square(store, image if on_host else None, S)
    tables = _square_tables(store, S)
    idx = torch.as_tensor(image).reshape(-1).to(device=store.device, dtype=torch.int32).contiguous()
    return ops.resample_u8(store.data, store.offsets_dev, store.sizes_dev, idx, None, 0, tables, tables, S, S, 0, 0, S, out=out)


def pajigsaw_pieces(store: Div2kImageStore, img_size: int) -> torch.Tensor:
    """The pre-cut pieces of one puzzle (``PajigsawPieces``, one stored image per piece) at the model's size, uint8 [n, 3, S, S]:
    what ``engine.puzzle_distances`` takes in pajigsaw.py's validation.  The reference's pieces make an 8-bit BGR -> LAB -> RGB
    round trip through cv2 on the way; that is not reproduced: the pieces are resized as stored."""
    return resize_images(store, list(range(len(store))), img_size)


class PajigsawIndex(NamedTuple):
    """``Pajigsaw.__init__``'s tables (data/datasets/pajigsaw_dataset.py:39-81) over fragment numbers: fragment f is the f-th
    fragment with ``degree == 0`` in the file's order, which is the order a store of the fragments has.  CSR tables are a pointer
    vector [rows + 1] and an index vector; all tensors int64."""
    im_path: list                # [F] the fragments' files, in store order
    im_names: list               # [m] sorted names of the images that have samples
    fragment: torch.Tensor       # [F, 3] (image: position in im_names or -1, row, col)
    samples: torch.Tensor        # [n] the fragments with a positive, stably sorted by (col, row)
    pos_ptr: torch.Tensor        # [F + 1] positives of every fragment, in the reference's order
    pos_idx: torch.Tensor
    neg_ptr: torch.Tensor        # [F + 1] in-image negatives
    neg_idx: torch.Tensor
    ent_ptr: torch.Tensor        # [m + 1] ``entries`` of every image of im_names
    ent_idx: torch.Tensor

    def to(self, device):
        return self._replace(**{k: v.to(device) for k, v in self._asdict().items() if torch.is_tensor(v)})


def _csr(rows):
    ptr = [0]
    for r in rows:
        ptr.append(ptr[-1] + len(r))
    return torch.tensor(ptr, dtype=torch.int64), torch.tensor([v for r in rows for v in r], dtype=torch.int64)


def pajigsaw_index(dataset: dict) -> PajigsawIndex:
    """The parsed ``{split}.json`` of the Pajigsaw data set -> ``PajigsawIndex``, in plain Python on the host: the fragments with
    ``degree == 0``; per fragment its positives (row or column neighbours at distance 1) and in-image negatives, skipping a second
    fragment with ``white_percentage > 0.85`` or the same ``im_path``; the samples are the fragments with at least one positive."""
    frags, per_image = [], {}
    for name in dataset:
        per_image[name] = []
        for frag in dataset[name]['Fragment1v1Rotate90']:
            if frag['degree'] == 0:
                per_image[name].append(len(frags))
                frags.append((name, frag))
    pos, neg = [[] for _ in frags], [[] for _ in frags]
    entries, samples = {}, []
    for name, members in per_image.items():
        for f in members:
            first = frags[f][1]
            for g in members:
                second = frags[g][1]
                if second['white_percentage'] > 0.85 or first['im_path'] == second['im_path']:
                    continue
                if first['col'] == second['col'] and abs(first['row'] - second['row']) == 1:
                    pos[f].append(g)
                elif first['row'] == second['row'] and abs(first['col'] - second['col']) == 1:
                    pos[f].append(g)
                else:
                    neg[f].append(g)
            if pos[f]:
                entries.setdefault(name, []).append(f)
                samples.append(f)
    im_names = sorted(entries)
    number = {name: k for k, name in enumerate(im_names)}
    samples = sorted(samples, key=lambda f: (frags[f][1]['col'], frags[f][1]['row']))          # stable, as the reference's sort
    fragment = torch.tensor([[number.get(name, -1), frag['row'], frag['col']] for name, frag in frags], dtype=torch.int64).reshape(-1, 3)
    return PajigsawIndex([frag['im_path'] for _, frag in frags], im_names, fragment, torch.tensor(samples, dtype=torch.int64),
                         *_csr(pos), *_csr(neg), *_csr([entries[name] for name in im_names]))


def _csr_choice(ptr: torch.Tensor, idx: torch.Tensor, row: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
    """random.choice(row's list) from uniforms ``t``: element min(floor(t len), len - 1); an empty list gives some valid element of
    ``idx`` (the caller discards it)."""
    start, length = ptr[row], ptr[row + 1] - ptr[row]
    pick = torch.minimum(torch.floor(t * length).to(torch.int64), length - 1).clamp_(min=0)
    return idx[(start + pick).clamp_(max=max(idx.numel() - 1, 0))] if idx.numel() else torch.zeros_like(row)


def pajigsaw_pair_plan(u: torch.Tensor, sample: torch.Tensor, index: PajigsawIndex):
    """The random choices of ``Pajigsaw.__getitem__`` (pajigsaw_dataset.py:87-131) for a whole batch at once, from uniform numbers
    ``u`` [B, 4] in [0, 1) (columns: positive draw, negative draw, the choice within the list, the other image) and the sample
    numbers ``sample`` [B] (positions in ``index.samples``): (first int64 [B], second int64 [B], labels fp32 [B, 4]), fragments by
    number.  Positive iff u0 < 0.75: second = positive[min(floor(u2 len), len - 1)], the label the side of ``first`` that ``second``
    lies on (same column, first above: [0, 1, 0, 0], below: [0, 0, 0, 1]; same row, first left: [1, 0, 0, 0], right: [0, 0, 1, 0]).
    Otherwise the label is zero and second is negative[...] by u2 if u1 < 0.5 and the fragment has negatives, else a fragment of
    another image: image k = min(floor(u3 (m - 1)), m - 2) of the m images, stepping over the sample's own, and entries[image][...]
    by u2 (the reference redraws until the image differs: one draw of the same distribution).  Torch operations on the device of
    ``u``; ``index`` must live there (``index.to``)."""
    m = len(index.im_names)
    if m < 2:
        raise ValueError(f'pajigsaw_pair_plan: {m} image(s) with samples: a negative pair from another image needs two (the reference '
                         f'would draw for ever)')
    u = u.double()
    first = index.samples[sample.to(device=u.device, dtype=torch.int64)]
    positive = u[:, 0] < 0.75
    in_image = (u[:, 1] < 0.5) & (index.neg_ptr[first + 1] > index.neg_ptr[first])
    own = index.fragment[first, 0]
    k = torch.minimum(torch.floor(u[:, 3] * (m - 1)).to(torch.int64), torch.full_like(own, m - 2))
    other = k + (k >= own).to(torch.int64)
    second = torch.where(positive, _csr_choice(index.pos_ptr, index.pos_idx, first, u[:, 2]),
                         torch.where(in_image, _csr_choice(index.neg_ptr, index.neg_idx, first, u[:, 2]),
                                     _csr_choice(index.ent_ptr, index.ent_idx, other, u[:, 2])))
    r1, c1, r2, c2 = index.fragment[first, 1], index.fragment[first, 2], index.fragment[second, 1], index.fragment[second, 2]
    bin_ = torch.where(c1 == c2, torch.where(r1 < r2, 1, 3), torch.where(c1 < c2, 0, 2))
    labels = torch.nn.functional.one_hot(bin_, 4).float() * positive.float().unsqueeze(1)
    return first, second, labels


class PajigsawDeviceLoader(_DeviceLoader):
    """pajigsaw.py's training loader on the device: what ``get_dataloader('train')`` over ``Pajigsaw`` delivers, from a
    ``Div2kImageStore`` of the fragments in ``index.im_path``'s order, without a host copy or a sync per batch.  An epoch is a
    permutation (drawn on the device, the same on every rank) of the sample numbers, of which rank r takes every ``world``-th from
    r on; the last incomplete batch is dropped.  Each batch: uniforms -> ``pajigsaw_pair_plan`` -> ``ops.resample_u8`` of the first
    fragments into ``pairs[:, 0]`` and of the second ones into ``pairs[:, 1]``; it yields (pairs uint8 [B, 2, 3, S, S], labels fp32
    [B, 4]) for ``TrainStep.step``.  The transform is ``TwoImgSyncEval.normalize`` on each fragment (the reference hands the
    two-image transform to a one-image call, which raises; that is what it means)."""

    def __init__(self, store: Div2kImageStore, index: PajigsawIndex, batch_size: int, img_size: int, rank: int = 0, world: int = 1,
                 seed: int = 0):
        if len(index.im_path) != len(store):
            raise ValueError(f'the index names {len(index.im_path)} fragments, the store holds {len(store)} images')
        if len(index.im_names) < 2:
            raise ValueError(f'{len(index.im_names)} image(s) with samples: every sample can draw a fragment of another image, which needs '
                             f'two (the reference would draw for ever)')
        self.index, self.img_size = index.to(store.device), int(img_size)
        super().__init__(store, batch_size, 1, rank, world, seed)
        _require_square(store, None, self.img_size, index.im_path)
        self.tables = _square_tables(store, self.img_size)

    def __len__(self):
        return self.index.samples.numel() // self.world // self.batch_size

    def epoch_order(self) -> torch.Tensor:
        """The epoch's permutation of the sample numbers (int64 on the store's device), before sharding."""
        return torch.randperm(self.index.samples.numel(), generator=self._generator(0), device=self.store.device)

    def rank_indices(self) -> torch.Tensor:
        """[len(self), batch_size]: the sample number of every sample this rank sees in the epoch."""
        per_rank = self.index.samples.numel() // self.world
        mine = self.epoch_order()[self.rank::self.world][:per_rank]
        return mine[: len(self) * self.batch_size].view(len(self), self.batch_size)

    def plan(self, sample: torch.Tensor, generator: torch.Generator):
        """One batch's draws: the three tensors of ``pajigsaw_pair_plan``."""
        u = torch.rand(sample.numel(), 4, generator=generator, device=self.store.device)
        return pajigsaw_pair_plan(u, sample, self.index)

    def feed(self, first: torch.Tensor, second: torch.Tensor) -> torch.Tensor:
        """Fragment numbers [B], [B] -> uint8 pairs [B, 2, 3, S, S]: two resize launches, each into its half of the pairs."""
        S, st, t = self.img_size, self.store, self.tables
        pairs = torch.empty(first.numel(), 2, 3, S, S, dtype=torch.uint8, device=st.device)
        for half, frag in enumerate((first, second)):
            ops.resample_u8(st.data, st.offsets_dev, st.sizes_dev, frag.to(torch.int32), None, 0, t, t, S, S, 0, 0, S, out=pairs[:, half])
        return pairs

    def __iter__(self):
        g = self._generator(1 + self.rank)
        for sample in self.rank_indices():
            first, second, labels = self.plan(sample, g)
            yield self.feed(first, second), labels


class _WindowSource:
    """An image source of ``engine.pairwise_similarity`` that serves device tensors straight from a store: a callable
    ``(lo, hi) -> uint8 [hi - lo, 3, S, S]`` with ``__len__``; a subclass sets the per-image windows, the fill and the resize."""
    fill = 0

    def __init__(self, store: Div2kImageStore, img_size: int, resized: int, windows):
        self.store, self.img_size, self.resized = store, int(img_size), int(resized)
        self.crop = _half(self.resized - self.img_size)
        self.windows = torch.tensor(windows, dtype=torch.int32).reshape(-1, 4).to(store.device)
        self.tables = ops.resample_tables([self.img_size], self.resized, store.device)

    def __len__(self):
        return len(self.store)

    def __call__(self, lo: int, hi: int) -> torch.Tensor:
        lo, hi = int(lo), int(hi)
        if not 0 <= lo < hi <= len(self):
            raise IndexError(f'images {lo}..{hi} of {len(self)}')
        st, t = self.store, self.tables
        image = torch.arange(lo, hi, dtype=torch.int32, device=st.device)
        return ops.resample_u8(st.data, st.offsets_dev, st.sizes_dev, image, self.windows[lo:hi], self.fill, t, t, self.resized,
                               self.resized, self.crop, self.crop, self.img_size)


class CenterCropSource(_WindowSource):
    """HisFrag's evaluation transform (hisfrag.py:83-93) from the store: torchvision's ``CenterCrop(S)`` - an axis shorter than S is
    padded with 0, (S - len) // 2 in front and (S - len + 1) // 2 behind; otherwise the crop starts at int(round((len - S) / 2.0))."""

    def __init__(self, store: Div2kImageStore, img_size: int):
        S = int(img_size)
        origin = lambda n: -((S - n) // 2) if n < S else _half(n - S)
        super().__init__(store, S, S, [[origin(h), origin(w), S, S] for h, w in store.sizes.tolist()])


class MichiganEvalSource(_WindowSource):
    """michigan.py's evaluation transform (michigan.py:90-96) from the store: ``PadCenterCrop(S, pad_if_needed, fill 255)`` - an axis
    shorter than S is padded by S - len on both sides, then torchvision's centre crop - then ``Resize(R = int(1.15 S))`` and
    ``CenterCrop(S)`` at int(round((R - S) / 2.0)); only the cropped region of the resized image is computed."""
    fill = 255

    def __init__(self, store: Div2kImageStore, img_size: int):
        S = int(img_size)
        origin = lambda n: _half(S - n) - (S - n) if n < S else _half(n - S)
        super().__init__(store, S, int(S * 1.15), [[origin(h), origin(w), S, S] for h, w in store.sizes.tolist()])
