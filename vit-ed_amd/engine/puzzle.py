"""Puzzle evaluation (evaluation.py:100-133, solver_driver.py, paikin_tal_solver/) for puzzles of one image, fixed size: the piece
distances from the model's logits, the Paikin-Tal solver with its compatibilities on the device, and the reference's accuracies; and
the classical baseline of solver_driver.py around the same solver - the image cut into eroded pieces, the prediction-based border
distances of the pieces' pixels, the solved board as an image.  Type-1 puzzles (orientation known) take distances [4, n, n]; type-2
puzzles (any side of a piece may meet any side of another; the solver assigns each piece a rotation) take distances [4, n, n, 4] of
the pixel path or of the model (``puzzle_type=2``), and every function here tells the two apart by that rank or by
``PuzzleSolution.rotations``.  Puzzles of unknown size and the pooled pieces of several images (``solve_puzzle(dq, None, ...)``) are
solved by ``puzzle_mixed``."""
from __future__ import annotations

import heapq
from typing import NamedTuple

import torch

from .. import ops
from .similarity import _ImageSource


PUZZLE_SIDES = ('top', 'right', 'bottom', 'left')          # PuzzlePieceSide values 0..3; side s touches side (s + 2) % 4
_SIDE_STEP = ((-1, 0), (0, 1), (1, 0), (0, -1))
_DQ_UNSET = 2 ** 31 - 1                                     # the reference's fill of its distance arrays (the diagonal)


def _ordered_block_pairs(a0, a1, n, dev):
    """Pairs (i, j), i in [a0, a1), j in [0, n), j != i, row-major."""
    ii = torch.arange(a0, a1, device=dev).view(-1, 1).expand(a1 - a0, n)
    jj = torch.arange(0, n, device=dev).view(1, -1).expand(a1 - a0, n)
    keep = jj != ii
    return ii[keep], jj[keep]


@torch.no_grad()
def puzzle_distances(model, pieces, *, pair_batch: int = 1024, amp: bool = True, block: int = 128, return_logits: bool = False,
                     puzzle_type: int = 1):
    """The reference's integer piece distances ``Dq`` int32 [4, n, n] on the device (evaluation.py:100-133 feeding
    inter_piece_distance.py:206-223): Dq[s, i, j] is the distance of side s of piece i (top 0, right 1, bottom 2, left 3) to the
    complementary side of piece j, from the model's logits of the ordered pair (i, j) (bin (s + 3) % 4), quantised as
    uint32(trunc(fp32(fp32(1 - sigmoid(logit)) * 1000))).  The diagonal holds 2^31 - 1 (never read).

    ``pieces``: the n pieces of one puzzle at model size, uint8 [n, 3, S, S] (normalised in the patch-embedding kernel) or
    normalised float, on the host or the device.  The encoder and the image-2 token cache run once per piece; the decoder runs on
    all n (n - 1) ordered pairs, ``pair_batch`` at a time, row block by row block of ``block`` pieces, and every batch's logits
    are quantised and scattered into Dq on the device.  ``return_logits`` also returns the fp32 logits [n, n, 4] (diagonal 0).

    ``puzzle_type=2`` (pieces of unknown rotation): Dq2 int32 [4, n, n, 4] over all 16 side pairings, what
    ``solve_puzzle`` solves as a type-2 puzzle.  Dq2[si, i, j, sj] is bin (si + 3) % 4 of the pair (piece i, piece j turned by
    k = (si + 2 - sj) % 4 clockwise quarter turns, so that its side sj faces side si), quantised as above; Dq2[s, :, :, (s + 2) % 4]
    is the type-1 Dq[s], bit for bit at equal ``pair_batch`` and ``block``.  The encoder still runs once per piece; the image-2 token
    cache is built for the 4 n turned pieces from the upright ones, and within a row block the pairs run turn by turn, each turn
    batched on its own.  ``return_logits`` then returns fp32 [n, n, 4, 4], indexed [i, j, k, bin] (diagonal 0)."""
    if puzzle_type not in (1, 2):
        raise ValueError(f'puzzle_distances: puzzle_type must be 1 or 2, got {puzzle_type!r}')
    if not getattr(model, 'supports_pair_cache', False):
        raise TypeError('puzzle_distances needs the HIP model (VisionTransformerCustom): it runs on the pair caches')
    if getattr(model, 'num_classes', 4) != 4:
        raise ValueError(f'puzzle_distances needs the 4-bin puzzle head, the model has {model.num_classes} outputs')
    dev = next(model.parameters()).device
    src = _ImageSource(pieces, None, dev)
    n = src.n
    if n < 2:
        raise ValueError('a puzzle needs at least two pieces')
    type2 = puzzle_type == 2
    turns = (0, 1, 2, 3) if type2 else (0,)
    dq = torch.full((4, n, n, 4) if type2 else (4, n, n), _DQ_UNSET, dtype=torch.int32, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    logits = torch.zeros((n, n, 4, 4) if type2 else (n, n, 4), dtype=torch.float32, device=dev) if return_logits else None
    dtype_ctx = lambda: torch.autocast(dev.type, dtype=torch.bfloat16, enabled=amp)
    was_training = model.training
    model.eval()
    try:
        with dtype_ctx():
            if type2:                                                       # once per piece and turn: rows k n + j, from one upright copy
                upright = src.block(0, n)
                caches = [model.cache_image2_tokens(upright, turn=k) for k in turns]
                tokens2 = torch.cat([c[0] for c in caches])
                q0 = None if caches[0][1] is None else torch.cat([c[1] for c in caches])
                del caches, upright
            else:
                tokens2, q0 = model.cache_image2_tokens(src.block(0, n))    # once per piece
        for a0 in range(0, n, block):
            a1 = min(a0 + block, n)
            with dtype_ctx():
                feats = model(src.block(a0, a1), forward_first_part=True)   # encoder once per piece
                kvs = model.cache_context_kv(feats)
            del feats
            ii, jj = _ordered_block_pairs(a0, a1, n, dev)
            for k in turns:                                                 # k = 0: the launches of a type-1 puzzle
                for p0 in range(0, ii.numel(), pair_batch):
                    i_sub, j_sub = ii[p0:p0 + pair_batch], jj[p0:p0 + pair_batch]
                    jt_sub = j_sub + k * n if k else j_sub
                    with dtype_ctx():
                        out = model.forward_pairs_cached(tokens2, jt_sub, kvs, i_sub - a0, q0)
                    out = out.float().reshape(-1, 4).contiguous()
                    if type2:
                        ops.puzzle_distances2_from_logits(out, i_sub.contiguous(), jt_sub.contiguous(), dq, bad)
                    else:
                        ops.puzzle_distances_from_logits(out, i_sub.contiguous(), j_sub.contiguous(), dq, bad)
                    if logits is not None:
                        if type2:
                            logits[i_sub, j_sub, k] = out
                        else:
                            logits[i_sub, j_sub] = out
            del kvs
    finally:
        model.train(was_training)
    if int(bad.item()):
        raise RuntimeError('puzzle_distances: a pair index fell outside the puzzle (internal error)')
    return (dq, logits) if return_logits else dq


class PuzzleCompatibility:
    """The Paikin-Tal compatibility state of one puzzle on the device (InterPieceDistance): built from Dq int32 [4, n, n] (type 1) by
    ``vited_puzzle_compat_init`` or from Dq2 int32 [4, n, n, 4] (type 2, ``puzzle_type`` 2) by ``vited_puzzle_compat2_init``;
    ``recalc`` and ``best_slot`` are the solver's two pool-empty steps.  Tensors, type 1: min_d, second_d int64 [n, 4], candidate,
    best_buddy int32 [n, 4], compat, mutual float32 [4, n, n], start_count int32 [n], start_total float32 [n], start_order int32 [n].
    Type 2: compat, mutual float32 [4, n, n, 4] ([si, i, j, sj]), candidate, best_buddy int32 [n, 4, 2] ((piece, side) or (-1, -1)) and
    min_count int32 [n, 4] beside the others."""

    def __init__(self, dq: torch.Tensor):
        self.dq = dq.to(torch.int32).contiguous()
        if self.dq.dim() not in (3, 4):
            raise ValueError(f'PuzzleCompatibility: distances must be [4, n, n] or [4, n, n, 4], got shape {list(self.dq.shape)}')
        self.puzzle_type = 2 if self.dq.dim() == 4 else 1
        self.n = self.dq.shape[1]
        self.state = ops.puzzle_compat2_init(self.dq) if self.puzzle_type == 2 else ops.puzzle_compat_init(self.dq)
        dev = self.dq.device
        self._placed = torch.empty(self.n, dtype=torch.int32, device=dev)
        self.changed = torch.zeros(self.n, dtype=torch.int32, device=dev)
        self._word = torch.empty(1, dtype=torch.int64, device=dev)

    def __getattr__(self, name):
        state = self.__dict__.get('state')
        if state is not None and name in state:
            return state[name]
        raise AttributeError(name)

    def recalc(self, placed) -> torch.Tensor:
        """recalculate_remaining_piece_compatibilities for the boolean mask ``placed`` [n]; returns the changed flags (device)."""
        self._placed.copy_(torch.as_tensor(placed, dtype=torch.int32))
        (ops.puzzle_compat2_recalc if self.puzzle_type == 2 else ops.puzzle_compat_recalc)(self.dq, self._placed, self.state, self.changed)
        return self.changed

    def mutual_at(self, lookups):
        """The mutual compatibilities the placement loop asks for, float32 [m] (numpy), fetched on the device
        (``vited_puzzle_mutual_gather``): ``lookups`` host integers [m, 3] = (side, p, q) -> mutual[side, p, q] (type 1) or [m, 4] =
        (side_p, p, q, side_q) -> mutual[side_p, p, q, side_q] (type 2).  One launch and one read through a small pinned buffer
        (the flag word in front of the m values); no copy of M is made.  An index outside the tensor raises IndexError."""
        import numpy as np
        width = 4 if self.puzzle_type == 2 else 3
        look = np.ascontiguousarray(lookups, dtype=np.int32).reshape(-1, width)
        m = look.shape[0]
        if m == 0:
            return np.empty(0, dtype=np.float32)
        room = self.__dict__.get('_gather')
        if room is None or room[0].shape[0] < m:
            cap, dev = max(64, 2 * m), self.dq.device
            room = (torch.empty((cap, width), dtype=torch.int32).pin_memory(), torch.empty((cap, width), dtype=torch.int32, device=dev),
                    torch.zeros(cap + 1, dtype=torch.float32, device=dev), torch.empty(cap + 1, dtype=torch.float32).pin_memory())
            self._gather = room
        look_host, look_dev, words_dev, words_host = room
        look_host[:m].copy_(torch.from_numpy(look))
        look_dev[:m].copy_(look_host[:m], non_blocking=True)
        bad = words_dev[:1].view(torch.int32)                   # stays zero from one call to the next: a set flag raises below
        ops.puzzle_mutual_gather(self.mutual, look_dev[:m], out=words_dev[1:m + 1], bad=bad)
        words_host[:m + 1].copy_(words_dev[:m + 1], non_blocking=True)
        torch.cuda.current_stream(self.dq.device).synchronize()
        if int(words_host[:1].view(torch.int32)[0]):
            bad.zero_()
            raise IndexError(f'mutual_at: a lookup fell outside the {self.n} pieces or the 4 sides')
        return words_host[1:m + 1].numpy().copy()

    def best_slot(self, placed, slot_piece, slot_side, value: bool = True):
        """Type 1: (piece, slot index, value) of the first maximum of mutual[(slot_side[k] + 2) % 4, p, slot_piece[k]] over unplaced p
        ascending x slots k in list order.  Type 2: (piece, slot index, side of the piece, value) of the first maximum of
        mutual[side, p, slot_piece[k], slot_side[k]] over unplaced p ascending x slots k in list order x side 0..3.  ``value=False``
        leaves the value out (the caller fetches it with ``mutual_at``)."""
        dev = self.dq.device
        self._placed.copy_(torch.as_tensor(placed, dtype=torch.int32))
        sp = torch.as_tensor(slot_piece, dtype=torch.int32).to(dev)
        ss = torch.as_tensor(slot_side, dtype=torch.int32).to(dev)
        if self.puzzle_type == 2:
            ops.puzzle_best_slot2(self.mutual, self._placed, sp, ss, out=self._word)
            hit = ops.puzzle_unpack_slot2(int(self._word.item()), sp.numel())
            if hit is None:
                raise RuntimeError('best_slot: no unplaced piece')
            p, k, side = hit
            if not value:
                return p, k, side
            return p, k, side, float(self.mutual[side, p, int(slot_piece[k]), int(slot_side[k])])
        ops.puzzle_best_slot(self.mutual, self._placed, sp, ss, out=self._word)
        hit = ops.puzzle_unpack_slot(int(self._word.item()), sp.numel())
        if hit is None:
            raise RuntimeError('best_slot: no unplaced piece')
        p, k = hit
        if not value:
            return p, k
        return p, k, float(self.mutual[(int(slot_side[k]) + 2) % 4, p, int(slot_piece[k])])


class PuzzleSolution(NamedTuple):
    locations: 'object'         # int64 [n, 2]: (row, col) of every piece, the placed block's top-left corner at (0, 0)
    board_locations: 'object'   # int64 [n, 2]: where the solver put each piece on its n x n board (seed at (n // 2, n // 2))
    order: 'object'             # int64 [n]: placement order, the seed first
    recalcs: int                # times the best-buddy pool ran empty and the compatibilities were recalculated
    grid: 'object'              # int64 [rows, cols]: the piece at each cell, -1 for none
    rotations: 'object' = None  # type 2: int64 [n], the quarter turns 0..3 the solver gave each piece (numpy.rot90's k); type 1: None


class _BuddyHeapEntry:
    """A best-buddy / open-slot pairing of the solver's heap (solver.py:32-64): heapq pops the largest mutual compatibility, ties
    falling out of the heap's own structure, so the push order and this one comparison must be the reference's."""
    __slots__ = ('compat', 'piece', 'piece_side', 'neighbor', 'neighbor_side', 'location')

    def __init__(self, compat, piece, piece_side, neighbor, neighbor_side, location):
        self.compat, self.piece, self.piece_side = compat, piece, piece_side
        self.neighbor, self.neighbor_side, self.location = neighbor, neighbor_side, location

    def __lt__(self, other):
        return self.compat > other.compat


def solve_puzzle(distances: torch.Tensor, grid_size=None, *, numb_puzzles: int = 1, new_board_mutual_compatibility: float = 0.5,
                 mutual_lookup: str | None = None) -> PuzzleSolution:
    """Paikin-Tal placement (PaikinTalSolver, solver.py) of one puzzle of ``grid_size`` = (rows, cols) pieces, making the reference's
    decisions in the reference's order: the seed from the start ordering at the board centre, best buddies pooled as pieces are
    placed, the best-buddy heap popped until it yields a placeable entry, and - whenever the pool is empty - a device recalculation
    of the compatibilities followed by a device scan of every unplaced piece against every open slot.  The host keeps a mirror of
    the mutual compatibility for the heap's lookups, fetched again by the first lookup after a recalculation.

    ``distances`` int32 [4, n, n] (``puzzle_distances``, ``puzzle_pixel_distances``) is a type-1 puzzle: only complementary sides
    meet.  ``distances`` int32 [4, n, n, 4] (``puzzle_pixel_distances(pieces, puzzle_type=2)``) is a type-2 puzzle: every open slot
    is tried against all four sides of a piece, the seed lies at rotation 0, each placed piece gets the rotation of
    PuzzlePiece._calculate_placed_piece_rotation, and the slots it opens carry its unrotated sides
    (_get_neighbor_locations_and_sides); ``PuzzleSolution.rotations`` holds the quarter turns.

    ``grid_size=None`` solves without dimensions (``fixed_puzzle_dimensions=None``: every slot passes the dimension check), and
    ``numb_puzzles`` > 1 - which needs ``grid_size=None``, as in the reference - solves the pooled pieces of several images, spawning a
    board whenever the found piece's mutual compatibility lies below ``new_board_mutual_compatibility`` while boards are left to
    spawn.  Both return a ``PuzzleBoards`` (a ``PuzzleSolution`` with the boards and their extents) and read the
    mutual compatibility by device lookups (``mutual_lookup='gather'``, ``PuzzleCompatibility.mutual_at``) instead of the host mirror
    (``'mirror'``, kept for comparison).  With ``grid_size`` given, nothing of this runs."""
    from . import puzzle_mixed
    mutual_lookup = puzzle_mixed.check_solve_arguments(grid_size, numb_puzzles, mutual_lookup)
    if grid_size is None:
        return puzzle_mixed.solve_open_puzzle(distances, numb_puzzles, new_board_mutual_compatibility, mutual_lookup)
    import numpy as np
    rows, cols = int(grid_size[0]), int(grid_size[1])
    n = distances.shape[1] if distances.dim() > 1 else 0
    type2 = distances.dim() == 4
    if rows * cols != n or tuple(distances.shape) != ((4, n, n, 4) if type2 else (4, n, n)):
        raise ValueError(f'distances {tuple(distances.shape)} do not describe a {rows} x {cols} puzzle')
    comp = PuzzleCompatibility(distances)
    mirror = [None]                                         # M on the host: dropped by a recalculation, fetched again by the next lookup
    best_buddy = comp.best_buddy.cpu().numpy().reshape(n, 4, -1)[:, :, 0]       # the buddy's piece id, either type
    seed = int(comp.start_order[0].item())
    # the sides of a piece that may meet a slot whose placed neighbour shows side s, and the mutual compatibility of the pairing
    sides_for = (lambda s: (0, 1, 2, 3)) if type2 else (lambda s: ((s + 2) % 4,))

    def m(p, ps, q, qs):
        if mirror[0] is None:
            mirror[0] = comp.mutual.cpu().numpy()
        return float(mirror[0][ps, p, q, qs] if type2 else mirror[0][ps, p, q])

    placed = np.zeros(n, dtype=bool)
    occupied = np.zeros((n, n), dtype=bool)                # the reference's board: n x n, indexed as numpy indexes it
    board_loc = np.full((n, 2), -1, dtype=np.int64)
    rotation = np.zeros(n, dtype=np.int64)                 # quarter turns; stays 0 throughout a type-1 puzzle
    top_left, bottom_right = [n // 2, n // 2], [n // 2, n // 2]
    open_slots = []                                         # (location, piece, unrotated side of that piece facing the slot), list order
    pool = {}                                               # best buddies waiting, insertion ordered
    heap = []
    order = []
    recalcs = 0

    def fits(loc):
        for d, size in ((0, rows), (1, cols)):
            if loc[d] - top_left[d] + 1 > size or bottom_right[d] - loc[d] + 1 > size:
                return False
        return True

    def slot_open(loc):
        return not occupied[loc] and fits(loc)

    def put(piece, loc):
        board_loc[piece] = loc
        occupied[loc] = True
        placed[piece] = True
        order.append(piece)

    def add_best_buddies(piece):
        for s in range(4):
            bb = int(best_buddy[piece, s])
            if bb < 0 or placed[bb] or bb in pool:
                continue
            pool[bb] = None
            for loc, q, side in open_slots:
                for bb_side in sides_for(side):
                    heapq.heappush(heap, _BuddyHeapEntry(m(bb, bb_side, q, side), bb, bb_side, q, side, loc))

    def open_slots_around(piece):
        r, c = board_loc[piece]
        for d, (dr, dc) in enumerate(_SIDE_STEP):
            loc, s = (int(r + dr), int(c + dc)), int(d - rotation[piece]) % 4
            if slot_open(loc):
                open_slots.append((loc, piece, s))
                for bb in list(pool):
                    for bb_side in sides_for(s):
                        heapq.heappush(heap, _BuddyHeapEntry(m(piece, s, bb, bb_side), bb, bb_side, piece, s, loc))

    put(seed, (n // 2, n // 2))
    add_best_buddies(seed)
    open_slots_around(seed)
    while not placed.all():
        if pool:
            while True:
                e = heapq.heappop(heap)
                if not placed[e.piece] and slot_open(e.location):
                    break
            piece, piece_side, neighbor, neighbor_side, loc, from_pool = e.piece, e.piece_side, e.neighbor, e.neighbor_side, e.location, True
        else:
            recalcs += 1
            comp.recalc(placed)
            mirror[0] = None
            valid = [k for k, (loc, _, _) in enumerate(open_slots) if slot_open(loc)]
            hit = comp.best_slot(placed, [open_slots[v][1] for v in valid], [open_slots[v][2] for v in valid])
            piece, (loc, neighbor, neighbor_side), from_pool = hit[0], open_slots[valid[hit[1]]], False
            piece_side = hit[2] if type2 else (neighbor_side + 2) % 4
        rotation[piece] = (rotation[neighbor] + (neighbor_side + 2) % 4 - piece_side) % 4
        for d in range(2):
            if top_left[d] > loc[d]:
                top_left[d] = loc[d]
            elif bottom_right[d] < loc[d]:
                bottom_right[d] = loc[d]
        put(piece, loc)
        open_slots = [slot for slot in open_slots if slot[0] != loc]
        if from_pool:
            del pool[piece]
        add_best_buddies(piece)
        open_slots_around(piece)

    locations = board_loc - board_loc.min(axis=0)
    shape = locations.max(axis=0) + 1
    grid = np.full((int(shape[0]), int(shape[1])), -1, dtype=np.int64)
    grid[locations[:, 0], locations[:, 1]] = np.arange(n)
    return PuzzleSolution(locations, board_loc, np.array(order, dtype=np.int64), recalcs, grid, rotation if type2 else None)


def puzzle_accuracy(solution: PuzzleSolution, true_locations, *, true_puzzle=None) -> dict:
    """The accuracies PuzzleResultsCollection.collect_results reports for one solved puzzle (puzzle_importer.py:779-844, the rules
    of :985-1150 and :1386-1520), every piece from the one original puzzle: ``Direct_Standard`` (pieces at their true cell / n),
    ``Direct_Modified`` (the same, best over the origins the reference's search from the top-left corner offers), ``neighbor``
    (sides whose neighbour - or board edge - is the true one / 4n) and ``perfect``.  ``true_locations`` int [n, 2]: where piece i
    belongs in the original rows x cols grid.

    A type-2 solution (``solution.rotations`` is not None) follows the reference's type-2 rules (:558-598, :985-1058): a piece at its
    true cell counts only at rotation 0 - otherwise it is a "wrong rotation", and the dict gains ``'wrong_rotation'``, their number
    under the standard origin; side s of a piece turned by r looks at the cell in direction (s + r) % 4, and a true neighbour found
    there counts only when both pieces carry the same rotation.

    ``true_puzzle`` int [n] (the image each piece came from; ``true_locations`` then lie in that image's grid) scores a mixed-bag
    solution (``puzzle_mixed.several_puzzle_accuracy``): the same keys, each a list with one entry per scored original puzzle."""
    import numpy as np
    if true_puzzle is not None:
        from .puzzle_mixed import several_puzzle_accuracy
        return several_puzzle_accuracy(solution, true_locations, true_puzzle)
    if getattr(solution, 'numb_boards', 1) > 1:
        raise ValueError('puzzle_accuracy: a solution of several boards is scored with true_puzzle, the image each piece came from')
    true = np.asarray(true_locations, dtype=np.int64)
    loc = np.asarray(solution.locations, dtype=np.int64)
    n = true.shape[0]
    t_rows, t_cols = int(true[:, 0].max()) + 1, int(true[:, 1].max()) + 1
    orig_id = true[:, 0] * t_cols + true[:, 1]
    g_rows, g_cols = int(loc[:, 0].max()) + 1, int(loc[:, 1].max()) + 1
    placed_id = np.full((g_rows, g_cols), -1, dtype=np.int64)
    placed_id[loc[:, 0], loc[:, 1]] = orig_id

    rot = None if getattr(solution, 'rotations', None) is None else np.asarray(solution.rotations, dtype=np.int64) % 4
    upright = np.ones(n, dtype=bool) if rot is None else rot == 0

    def correct_at(origin):
        return int((np.all(loc == true + np.asarray(origin), axis=1) & upright).sum())

    standard = correct_at((0, 0))
    # the reference's breadth-first search for the candidate origins (puzzle_importer.py:1081-1138)
    frontier, explored, found = [(0, 0)], [], None
    while found is None or (frontier and frontier[0][0] + frontier[0][1] <= found):
        cur = frontier.pop(0)
        explored.append(cur)
        if found is None and placed_id[cur] != -1:
            found = cur[0] + cur[1]
        else:
            for nxt in ((cur[0] + 1, cur[1]), (cur[0], cur[1] + 1)):
                if nxt[0] < g_rows and nxt[1] < g_cols and nxt not in explored and nxt not in frontier:
                    frontier.append(nxt)
    modified = max(correct_at(origin) for origin in explored)

    placed_rot = np.zeros((g_rows, g_cols), dtype=np.int64)
    if rot is not None:
        placed_rot[loc[:, 0], loc[:, 1]] = rot
    neighbors = 0
    for p in range(n):
        for s, (dr, dc) in enumerate(_SIDE_STEP):
            tr, tc = true[p, 0] + dr, true[p, 1] + dc
            want = int(tr * t_cols + tc) if 0 <= tr < t_rows and 0 <= tc < t_cols else None
            lr, lc = _SIDE_STEP[s if rot is None else int(s + rot[p]) % 4]
            r, c = loc[p, 0] + lr, loc[p, 1] + lc
            inside = 0 <= r < g_rows and 0 <= c < g_cols
            got = int(placed_id[r, c]) if inside else -1
            same_turn = want is None or rot is None or bool(inside and placed_rot[r, c] == rot[p])
            neighbors += (None if got < 0 else got) == want and same_turn
    out = {'Direct_Standard': standard / n, 'Direct_Modified': modified / n, 'neighbor': neighbors / (4 * n), 'perfect': standard == n}
    if rot is not None:
        out['wrong_rotation'] = int((np.all(loc == true, axis=1) & ~upright).sum())
    return out


# ---- the classical baseline (solver_driver.py): cut, pixel distances, board --------------------------------------------------------
class PuzzleCut(NamedTuple):
    pieces: 'object'            # uint8 [n, We, We, 3] on the device, in the solver's order
    true_locations: 'object'    # int64 [n, 2] (host): the cell (row, col) each piece was cut from
    grid_size: tuple            # (rows, cols); of several images: a tuple of them
    piece_width: int            # P, the cell's width before the erosion crop
    true_puzzle: 'object' = None    # several images: int64 [n] (host), the image each piece was cut from; one image: None


def _several_images(image):
    return isinstance(image, (list, tuple)) and len(image) > 0 and getattr(image[0], 'ndim', None) == 3


def cut_puzzle(image, piece_width: int, erosion: float = 0., order=None) -> PuzzleCut:
    """Puzzle(0, path, piece_width, erosion=erosion).pieces on the device (puzzle_importer.py:182-232): ``image`` uint8 [H, W, 3] (any
    3-channel image: the colour conversion is the caller's) cut into (H // P) x (W // P) cells of the centred grid, each centre-cropped to
    We = min(ceil(P (1 - erosion)), P).  ``order`` (a permutation of the row-major cells, host integers) is the driver's
    random.shuffle made explicit: piece k is cell order[k].

    A list of images is a mixed bag: every image is cut as above, the pieces are pooled image after image (Puzzle(k, ...,
    starting_piece_id=...)) and ``order`` permutes the pool; ``true_puzzle`` tells the images apart and ``grid_size`` lists their grids."""
    import numpy as np
    P = int(piece_width)
    if P < 1:
        raise ValueError(f'cut_puzzle: piece_width must be positive, got {piece_width}')
    if _several_images(image):
        cuts = [cut_puzzle(one, P, erosion) for one in image]
        pieces = torch.cat([cut.pieces for cut in cuts])
        true = np.concatenate([cut.true_locations for cut in cuts])
        puzzle = np.concatenate([np.full(len(cut.true_locations), k, dtype=np.int64) for k, cut in enumerate(cuts)])
        if order is not None:
            pick = np.asarray(order.cpu() if isinstance(order, torch.Tensor) else order, dtype=np.int64)
            if pick.shape != puzzle.shape or not np.array_equal(np.sort(pick), np.arange(puzzle.size)):
                raise ValueError(f'cut_puzzle: order must be a permutation of the {puzzle.size} pooled pieces')
            pieces, true, puzzle = pieces.index_select(0, torch.from_numpy(np.array(pick)).to(pieces.device)).contiguous(), true[pick], puzzle[pick]
        return PuzzleCut(pieces, true, tuple(cut.grid_size for cut in cuts), P, puzzle)
    image = torch.as_tensor(image)
    if not image.is_cuda and torch.cuda.is_available():        # a host image is uploaded; without a GPU ops refuses it
        image = image.cuda()
    image = image.contiguous()
    rows, cols = (image.shape[0] // P, image.shape[1] // P) if image.dim() == 3 else (0, 0)
    pieces = ops.puzzle_cut(image, P, ops.puzzle_eroded_width(P, erosion), order)
    cell = np.arange(rows * cols) if order is None else np.asarray(order.cpu() if isinstance(order, torch.Tensor) else order, dtype=np.int64)
    return PuzzleCut(pieces, np.stack([cell // cols, cell % cols], axis=1).astype(np.int64), (rows, cols), P)


def puzzle_model_pieces(pieces, size: int):
    """The pieces of ``cut_puzzle`` at the model's size, uint8 [n, 3, size, size]: TwoImgSyncEval's Resize on each piece (Pillow's
    8-bit bilinear resample, bit for bit), the input of ``puzzle_distances``."""
    return ops.puzzle_resize_pieces(pieces, size)


def puzzle_pixel_distances(pieces, puzzle_type: int = 1):
    """Dq int32 [4, n, n] of PuzzlePiece.calculate_asymmetric_distance (puzzle_piece.py:535-609) over all ordered pairs and sides of
    the pieces uint8 [n, We, We, 3] of ``cut_puzzle``: what ``solve_puzzle`` takes, as it takes ``puzzle_distances``' .
    ``puzzle_type=2``: Dq2 int32 [4, n, n, 4] over all 16 side pairings, [si, i, j, sj], which ``solve_puzzle`` solves as a type-2
    puzzle."""
    return ops.puzzle_pixel_distances(pieces, puzzle_type=puzzle_type)


def _reconstruct_boards(pieces, solution, true_locations, piece_width, marker):
    """One board per solved board of a ``PuzzleBoards``, each cropped to its extents.  ``vited_puzzle_assemble`` draws a board that its
    pieces fill, so every empty cell of the extent gets a black piece whose true location is that cell (no frame): the reference's
    black background."""
    import numpy as np
    true = np.asarray(true_locations, dtype=np.int64)
    loc_all = np.asarray(solution.locations, dtype=np.int64)
    boards, out = np.asarray(solution.boards), []
    for b in range(solution.numb_boards):
        on = np.flatnonzero(boards == b)
        loc = loc_all[on]
        R, C = int(loc[:, 0].max()) + 1, int(loc[:, 1].max()) + 1
        filled = np.zeros((R, C), dtype=bool)
        filled[loc[:, 0], loc[:, 1]] = True
        empty = np.argwhere(~filled).astype(np.int64)
        sub = pieces.index_select(0, torch.from_numpy(on).to(pieces.device))
        if len(empty):
            sub = torch.cat([sub, sub.new_zeros((len(empty),) + tuple(sub.shape[1:]))])
        sub = sub.contiguous()
        at, want = np.concatenate([loc, empty]), np.concatenate([true[on], empty])
        if solution.rotations is not None:
            turns = np.concatenate([np.asarray(solution.rotations, dtype=np.int64)[on], np.zeros(len(empty), dtype=np.int64)])
            out.append(ops.puzzle_assemble2(sub, at, turns, want, piece_width, marker))
        else:
            out.append(ops.puzzle_assemble(sub, at, want, piece_width, marker))
    return out


def reconstruct_puzzle(pieces, solution, true_locations, piece_width: int, marker=None):
    """Puzzle.reconstruct_from_pieces (puzzle_importer.py:265-321, :448-473): the board uint8 [R P, C P, 3] of the pieces at
    ``solution.locations`` (a ``PuzzleSolution``, or the locations themselves).  With ``marker`` (three bytes; the reference's is BGR
    (0, 0, 255)) every piece away from its true location is framed, which needs (P - We) // 2 >= 1.  A piece of a type-2 solution
    enters as numpy.rot90(piece, rotation); the frame still goes by the location alone, as insert_piece_into_image draws it.

    A ``PuzzleBoards`` (several boards, or one of unknown extents) gives a list: one board image per solved board, in board order, each
    cropped to that board's extents, black where no piece lies."""
    if getattr(solution, 'boards', None) is not None:
        return _reconstruct_boards(pieces, solution, true_locations, piece_width, marker)
    rotations = getattr(solution, 'rotations', None)
    if rotations is not None:
        return ops.puzzle_assemble2(pieces, solution.locations, rotations, true_locations, piece_width, marker)
    return ops.puzzle_assemble(pieces, getattr(solution, 'locations', solution), true_locations, piece_width, marker)


def _solve_cut(cut, distances, marker, grid_size, numb_puzzles, new_board_mutual_compatibility, mutual_lookup):
    """Solver, accuracies and board(s) of a cut, shared by the two drivers.  One image: ``grid_size`` 'cut' is the cut's own grid, None
    the unknown-dimension form.  Several images: no dimensions, ``numb_puzzles`` boards (default: one per image)."""
    if cut.true_puzzle is not None:
        if grid_size not in ('cut', None):
            from .puzzle_mixed import SEVERAL_WITH_DIMENSIONS
            raise ValueError(SEVERAL_WITH_DIMENSIONS)
        grid_size, numb_puzzles = None, len(cut.grid_size) if numb_puzzles is None else numb_puzzles
    elif grid_size == 'cut':
        grid_size = cut.grid_size
    solution = solve_puzzle(distances, grid_size, numb_puzzles=1 if numb_puzzles is None else numb_puzzles,
                            new_board_mutual_compatibility=new_board_mutual_compatibility, mutual_lookup=mutual_lookup)
    board = reconstruct_puzzle(cut.pieces, solution, cut.true_locations, cut.piece_width, marker)
    return solution, puzzle_accuracy(solution, cut.true_locations, true_puzzle=cut.true_puzzle), board


def solve_pixel_puzzle(image, piece_width: int, erosion: float = 0., order=None, marker=None, puzzle_type: int = 1, *, grid_size='cut',
                       numb_puzzles=None, new_board_mutual_compatibility: float = 0.5, mutual_lookup=None):
    """One pass of solver_driver.py's loop on the device: cut, pixel distances, Paikin-Tal, accuracies, board.  Returns
    (``PuzzleSolution``, the dict of ``puzzle_accuracy``, board uint8 [R P, C P, 3]).  ``puzzle_type=2`` solves the pieces as a type-2
    puzzle (paikin_tal_tester.py's PuzzleType.type2): the pieces are cut upright, the solver is free to turn them.

    A list of images is solved as a mixed bag (``numb_puzzles`` boards, one per image unless given) and ``grid_size=None`` solves one
    image without its dimensions: both return (``PuzzleBoards``, the accuracies - per original puzzle for a list -, the list of board
    images, one per solved board)."""
    cut = cut_puzzle(image, piece_width, erosion, order)
    return _solve_cut(cut, puzzle_pixel_distances(cut.pieces, puzzle_type), marker, grid_size, numb_puzzles, new_board_mutual_compatibility,
                      mutual_lookup)


def solve_model_puzzle(model, image, piece_width: int, erosion: float = 0., order=None, marker=None, puzzle_type: int = 1, **distance_kw):
    """The learned twin of ``solve_pixel_puzzle``, evaluation.py's loop body on the device: cut, the pieces at the model's size, the
    model's distances, Paikin-Tal, accuracies, board.  Returns (``PuzzleSolution``, the dict of ``puzzle_accuracy``, board uint8
    [R P, C P, 3]).  ``puzzle_type=2`` scores all 16 side pairings through the model and solves the pieces as a type-2 puzzle;
    ``distance_kw`` (pair_batch, amp, block) goes to ``puzzle_distances``.  A list of images and ``grid_size=None`` as in
    ``solve_pixel_puzzle``, whose solver keywords (grid_size, numb_puzzles, new_board_mutual_compatibility, mutual_lookup) are taken
    out of ``distance_kw``."""
    if puzzle_type not in (1, 2):
        raise ValueError(f'solve_model_puzzle: puzzle_type must be 1 or 2, got {puzzle_type!r}')
    if distance_kw.get('return_logits'):
        raise ValueError('solve_model_puzzle: return_logits belongs to puzzle_distances, the driver returns the solution')
    solver_kw = (distance_kw.pop('grid_size', 'cut'), distance_kw.pop('numb_puzzles', None),
                 distance_kw.pop('new_board_mutual_compatibility', 0.5), distance_kw.pop('mutual_lookup', None))
    cut = cut_puzzle(image, piece_width, erosion, order)
    distances = puzzle_distances(model, puzzle_model_pieces(cut.pieces, model.img_size), puzzle_type=puzzle_type, **distance_kw)
    return _solve_cut(cut, distances, marker, *solver_kw)
