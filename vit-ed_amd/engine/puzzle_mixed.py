"""Mixed-bag and unknown-dimension puzzles: the two behaviours of PaikinTalSolver that the fixed-size placement
of ``puzzle.solve_puzzle`` leaves out - the pieces of several images solved together, a new board spawned whenever the best next
placement is weak (solver.py:244-252, :507-562), and one puzzle solved without its dimensions (``fixed_puzzle_dimensions=None``,
solver.py:427-443) - and the accuracies PuzzleResultsCollection reports when the pieces of one original puzzle lie on several solved
boards.  The placement loop reads the mutual compatibility through ``PuzzleCompatibility.mutual_at``: a handful of device lookups per
placed piece instead of a host copy of M."""
from __future__ import annotations

import heapq

from .puzzle import _SIDE_STEP, PuzzleCompatibility, PuzzleSolution, _BuddyHeapEntry

NEW_BOARD_MUTUAL_COMPATIBILITY = 0.5        # PaikinTalSolver.DEFAULT_MINIMUM_MUTUAL_COMPATIBILITY_FOR_NEW_BOARD
SEVERAL_WITH_DIMENSIONS = 'When specifying puzzle dimensions, only a single puzzle is allowed.'     # solver.py:175
NO_PUZZLE = 'At least a single puzzle is required.'                                                # solver.py:173


class PuzzleBoards(PuzzleSolution):
    """The ``PuzzleSolution`` of a solve without dimensions or with several boards: the six fields of a ``PuzzleSolution`` -
    ``locations`` relative to the top-left corner of the piece's own board, ``grid`` the grid of board 0 - and beside them
      boards        int64 [n]: the board each piece was placed on, boards numbered in the order they were spawned
      top_left, bottom_right   int64 [B, 2]: every board's extents on its n x n canvas, as PuzzleDimensions tracks them
      grids         list of B int64 [rows_b, cols_b]: the piece at each cell of every board, -1 for none
      spawns        int64 [B]: the index in ``order`` of every board's seed (0 for the first)
      spawn_from_heap   bool [B - 1]: whether the weak placement that spawned board b + 1 came off the best-buddy heap (True) or out of
                    the slot scan after a recalculation (False)."""

    def __new__(cls, locations, board_locations, order, recalcs, grid, rotations=None, *, boards, top_left, bottom_right, grids, spawns,
                spawn_from_heap):
        self = super().__new__(cls, locations, board_locations, order, recalcs, grid, rotations)
        self.boards, self.top_left, self.bottom_right, self.grids = boards, top_left, bottom_right, grids
        self.spawns, self.spawn_from_heap = spawns, spawn_from_heap
        return self

    @property
    def numb_boards(self):
        return len(self.grids)


def grow_extents(top_left, bottom_right, loc):
    """PaikinTalSolver._updated_puzzle_dimensions (solver.py:580-586) on the two corner lists, in place: per dimension the top-left
    corner moves, or else the bottom-right one."""
    for d in range(2):
        if top_left[d] > loc[d]:
            top_left[d] = loc[d]
        elif bottom_right[d] < loc[d]:
            bottom_right[d] = loc[d]


def check_solve_arguments(grid_size, numb_puzzles, mutual_lookup):
    """The constructor's refusals (solver.py:172-175) and the lookup mode: 'mirror' for a solve with dimensions unless asked otherwise,
    'gather' without them."""
    if numb_puzzles < 1:
        raise ValueError(NO_PUZZLE)
    if numb_puzzles > 1 and grid_size is not None:
        raise ValueError(SEVERAL_WITH_DIMENSIONS)
    if mutual_lookup is None:
        mutual_lookup = 'mirror' if grid_size is not None else 'gather'
    if mutual_lookup not in ('gather', 'mirror'):
        raise ValueError(f"solve_puzzle: mutual_lookup must be 'gather' or 'mirror', got {mutual_lookup!r}")
    if grid_size is not None and mutual_lookup != 'mirror':
        raise ValueError("solve_puzzle: a puzzle of given dimensions is solved on the host mirror; mutual_lookup='gather' belongs to "
                         'grid_size=None')
    return mutual_lookup


def solve_open_puzzle(distances, numb_puzzles: int = 1, new_board_mutual_compatibility: float = NEW_BOARD_MUTUAL_COMPATIBILITY,
                      mutual_lookup: str = 'gather') -> PuzzleBoards:
    """PaikinTalSolver(numb_puzzles, pieces, ..., new_board_mutual_compatibility, fixed_puzzle_dimensions=None).run(), decision for
    decision: every slot passes the dimension check; after each found piece, while fewer than ``numb_puzzles`` boards exist, a mutual
    compatibility below the threshold discards the piece (the heap entry popped for it is gone), resets the best-buddy pool and heap -
    not the open slots, which keep their order and their boards - and seeds a new board at its centre with the first unplaced piece of
    the start ordering.  The slot scan and the heap run over the open slots of all boards.  ``distances`` as in ``solve_puzzle``."""
    import numpy as np
    n = distances.shape[1] if distances.dim() > 1 else 0
    type2 = distances.dim() == 4
    if n < 2 or tuple(distances.shape) != ((4, n, n, 4) if type2 else (4, n, n)):
        raise ValueError(f'distances {tuple(distances.shape)} are neither [4, n, n] nor [4, n, n, 4]')
    comp = PuzzleCompatibility(distances)
    best_buddy = comp.best_buddy.cpu().numpy().reshape(n, 4, -1)[:, :, 0]
    start_order = comp.start_order.cpu().numpy()
    sides_for = (lambda s: (0, 1, 2, 3)) if type2 else (lambda s: ((s + 2) % 4,))
    mirror = [None]

    def fetch(lookups):
        """M[side_p, p, q, side_q] of every (side_p, p, q, side_q), type 1 dropping the last."""
        if not lookups:
            return ()
        if mutual_lookup == 'gather':
            return comp.mutual_at(lookups if type2 else [look[:3] for look in lookups])
        if mirror[0] is None:
            mirror[0] = comp.mutual.cpu().numpy()
        return [mirror[0][look] if type2 else mirror[0][look[:3]] for look in lookups]

    centre = (n // 2, n // 2)
    placed = np.zeros(n, dtype=bool)
    board_of = np.full(n, -1, dtype=np.int64)
    board_loc = np.full((n, 2), -1, dtype=np.int64)
    rotation = np.zeros(n, dtype=np.int64)
    taken, corners = [], []                                 # per board: the set of filled locations; [top_left, bottom_right]
    open_slots = []                                         # (board, location, piece, unrotated side facing the slot), list order
    pool, heap = {}, []
    order, spawns, spawn_from_heap = [], [], []
    recalcs = 0

    def slot_open(board, loc):
        return loc not in taken[board]                      # _check_board_dimensions passes everything without dimensions

    def grow(piece):
        """_add_best_buddies_to_pool then _update_open_slots: the heap entries in the reference's push order, their values in one fetch."""
        looks, entries = [], []
        for s in range(4):
            bb = int(best_buddy[piece, s])
            if bb < 0 or placed[bb] or bb in pool:
                continue
            pool[bb] = None
            for board, loc, q, side in open_slots:
                for bb_side in sides_for(side):
                    looks.append((bb_side, bb, q, side))
                    entries.append((bb, bb_side, q, side, (board, loc)))
        board, (r, c) = int(board_of[piece]), board_loc[piece]
        for d, (dr, dc) in enumerate(_SIDE_STEP):
            loc, s = (int(r + dr), int(c + dc)), int(d - rotation[piece]) % 4
            if slot_open(board, loc):
                open_slots.append((board, loc, piece, s))
                for bb in list(pool):
                    for bb_side in sides_for(s):
                        looks.append((s, piece, bb, bb_side))
                        entries.append((bb, bb_side, piece, s, (board, loc)))
        for value, entry in zip(fetch(looks), entries):
            heapq.heappush(heap, _BuddyHeapEntry(float(value), *entry))

    def put(piece, board, loc):
        board_of[piece], board_loc[piece] = board, loc
        taken[board].add(loc)
        placed[piece] = True
        order.append(piece)

    def place_seed():
        seed = next(int(p) for p in start_order if not placed[p])           # next_starting_piece(placed)
        taken.append(set())
        corners.append([list(centre), list(centre)])
        spawns.append(len(order))
        put(seed, len(taken) - 1, centre)
        grow(seed)

    place_seed()
    while not placed.all():
        if pool:
            while True:
                e = heapq.heappop(heap)
                if not placed[e.piece] and slot_open(*e.location):
                    break
            piece, piece_side, neighbor, neighbor_side, (board, loc), value, from_pool = (e.piece, e.piece_side, e.neighbor, e.neighbor_side,
                                                                                         e.location, e.compat, True)
        else:
            recalcs += 1
            comp.recalc(placed)
            mirror[0] = None
            valid = [slot for slot in open_slots if slot_open(slot[0], slot[1])]
            hit = comp.best_slot(placed, [slot[2] for slot in valid], [slot[3] for slot in valid], value=False)
            piece, (board, loc, neighbor, neighbor_side), from_pool = hit[0], valid[hit[1]], False
            piece_side = hit[2] if type2 else (neighbor_side + 2) % 4
            value = float(fetch([(piece_side, piece, neighbor, neighbor_side)])[0])
        if len(taken) < numb_puzzles and value < new_board_mutual_compatibility:
            pool, heap = {}, []
            spawn_from_heap.append(from_pool)
            place_seed()
            continue
        rotation[piece] = (rotation[neighbor] + (neighbor_side + 2) % 4 - piece_side) % 4
        grow_extents(corners[board][0], corners[board][1], loc)
        put(piece, board, loc)
        open_slots[:] = [slot for slot in open_slots if not (slot[0] == board and slot[1] == loc)]
        if from_pool:
            del pool[piece]
        grow(piece)

    locations = np.zeros((n, 2), dtype=np.int64)
    grids = []
    for b in range(len(taken)):
        on = np.flatnonzero(board_of == b)
        locations[on] = board_loc[on] - board_loc[on].min(axis=0)
        shape = locations[on].max(axis=0) + 1
        grid = np.full((int(shape[0]), int(shape[1])), -1, dtype=np.int64)
        grid[locations[on, 0], locations[on, 1]] = on
        grids.append(grid)
    return PuzzleBoards(locations, board_loc, np.array(order, dtype=np.int64), recalcs, grids[0], rotation if type2 else None,
                        boards=board_of, top_left=np.array([c[0] for c in corners], dtype=np.int64),
                        bottom_right=np.array([c[1] for c in corners], dtype=np.int64), grids=grids,
                        spawns=np.array(spawns, dtype=np.int64), spawn_from_heap=np.array(spawn_from_heap, dtype=bool))


def several_puzzle_accuracy(solution, true_locations, true_puzzle) -> dict:
    """PuzzleResultsCollection(...).calculate_accuracies(solved boards) / collect_results() (puzzle_importer.py:738-843) for pieces of
    several original puzzles: one entry per scored original puzzle in every list of the dict.

    The rules it restates.  The original puzzles present, ascending by id, are zipped with the solved boards in board order
    (:791): original puzzle number i is scored against board i and no other, and what the shorter list leaves over is not scored.
    On that board a piece of another puzzle is a "different puzzle" piece (:583): the direct accuracies divide the correct
    placements by (pieces of the original puzzle anywhere + different-puzzle pieces on the board) (:831-833), ``perfect`` asks for
    equality with that weight (:836); the modified origin is the candidate with the most correct placements
    (check_if_update_direct_accuracy: the weights do not depend on the origin).  The neighbour accuracy records a different-puzzle
    piece once per side (:1022-1025), so its weight is 4 (pieces of the original puzzle + 4 x different-puzzle pieces) (:840-841).
    A neighbour is the true one by its piece id, unique over all puzzles; type-2 rules as in ``puzzle_accuracy``."""
    import numpy as np
    true = np.asarray(true_locations, dtype=np.int64)
    loc = np.asarray(solution.locations, dtype=np.int64)
    puzzle = np.asarray(true_puzzle, dtype=np.int64)
    n = true.shape[0]
    if puzzle.shape != (n,) or loc.shape != (n, 2):
        raise ValueError(f'puzzle_accuracy: true_puzzle must be [{n}] and the solution hold {n} pieces, got {puzzle.shape} and {loc.shape}')
    boards = getattr(solution, 'boards', None)
    boards = np.zeros(n, dtype=np.int64) if boards is None else np.asarray(boards, dtype=np.int64)
    rotations = getattr(solution, 'rotations', None)
    rot = None if rotations is None else np.asarray(rotations, dtype=np.int64) % 4
    upright = np.ones(n, dtype=bool) if rot is None else rot == 0

    originals = sorted(set(puzzle.tolist()))
    cols_of = {k: int(true[puzzle == k, 1].max()) + 1 for k in originals}
    rows_of = {k: int(true[puzzle == k, 0].max()) + 1 for k in originals}
    first_id, nxt = {}, 0
    for k in originals:                                     # globally unique piece ids, Puzzle(starting_piece_id=...)
        first_id[k], nxt = nxt, nxt + rows_of[k] * cols_of[k]
    orig_id = np.array([first_id[k] + r * cols_of[k] + c for k, (r, c) in zip(puzzle.tolist(), true.tolist())], dtype=np.int64)

    out = {'Direct_Standard': [], 'Direct_Modified': [], 'neighbor': [], 'perfect': []}
    if rot is not None:
        out['wrong_rotation'] = []
    for k, b in zip(originals, sorted(set(boards.tolist()))):
        on = np.flatnonzero(boards == b)
        mine = on[puzzle[on] == k]
        different = int(on.size - mine.size)
        weight = different + int((puzzle == k).sum())
        g_rows, g_cols = int(loc[on, 0].max()) + 1, int(loc[on, 1].max()) + 1
        placed_id = np.full((g_rows, g_cols), -1, dtype=np.int64)
        placed_rot = np.zeros((g_rows, g_cols), dtype=np.int64)
        placed_id[loc[on, 0], loc[on, 1]] = orig_id[on]
        if rot is not None:
            placed_rot[loc[on, 0], loc[on, 1]] = rot[on]

        def correct_at(origin):
            return int((np.all(loc[mine] == true[mine] + np.asarray(origin), axis=1) & upright[mine]).sum())

        standard = correct_at((0, 0))
        frontier, explored, found = [(0, 0)], [], None      # the reference's breadth-first search (puzzle_importer.py:1103-1127)
        while found is None or (frontier and frontier[0][0] + frontier[0][1] <= found):
            cur = frontier.pop(0)
            explored.append(cur)
            if found is None and placed_id[cur] != -1:
                found = cur[0] + cur[1]
            else:
                for step in ((cur[0] + 1, cur[1]), (cur[0], cur[1] + 1)):
                    if step[0] < g_rows and step[1] < g_cols and step not in explored and step not in frontier:
                        frontier.append(step)
        modified = max(correct_at(origin) for origin in explored)

        neighbors = 0
        for p in mine:
            for s, (dr, dc) in enumerate(_SIDE_STEP):
                tr, tc = true[p, 0] + dr, true[p, 1] + dc
                inside_true = 0 <= tr < rows_of[k] and 0 <= tc < cols_of[k]
                want = int(first_id[k] + tr * cols_of[k] + tc) if inside_true else None
                lr, lc = _SIDE_STEP[s if rot is None else int(s + rot[p]) % 4]
                r, c = loc[p, 0] + lr, loc[p, 1] + lc
                inside = 0 <= r < g_rows and 0 <= c < g_cols
                got = int(placed_id[r, c]) if inside else -1
                same_turn = want is None or rot is None or bool(inside and placed_rot[r, c] == rot[p])
                neighbors += (None if got < 0 else got) == want and same_turn
        out['Direct_Standard'].append(standard / weight)
        out['Direct_Modified'].append(modified / weight)
        out['neighbor'].append(neighbors / (4 * (int((puzzle == k).sum()) + 4 * different)))
        out['perfect'].append(standard == weight)
        if rot is not None:
            out['wrong_rotation'].append(int((np.all(loc[mine] == true[mine], axis=1) & ~upright[mine]).sum()))
    return out
