"""The ranks of one swarm under the cell-owner partition (sca_partition_*) in ONE process, and a model of who owns what.  Helper module of
tests/test_partition_fuzz_cpu.py, tests/test_gpu_partition_fuzz.py and form_fuzz.cut_scene; no test in it.

The partition's entry points take plain device pointers, so `world` contexts in one process can play `world` ranks and hand each other's
packed buffers over directly (Ranks): a few hundred agents, deliberate scenes, every agent checked at every step against the rule-1 oracle run
of the whole swarm -- which does not depend on who holds what.

The model (Model) is written from the documentation of include/sca_hip.h and the head of sca_amd/csrc/sca_partition.hip.h, not from the
kernels: the grid's cell is a little larger than the largest neighbor_dist, cell(x) = floor(x * inv_cell) in float64, the cuts are moved onto
cell boundaries, rank r owns the cells [cell_cut[r], cell_cut[r + 1]) along the axis and holds copies of the agents in the one layer of cells
on either side of its slab where a peer exists (the halo).  Per step a rank sends each slab neighbour the records of its agents in its layer
next to that neighbour (by their old or their moved cell) or that leave to it, and the agents that leave."""
import math

import numpy as np

FAR = 1 << 62                                  # the open ends of the first and the last slab
HEADER_INTS = 4                                # n_halo, n_mig, cap_halo, cap_mig: the first 16 bytes of a message


def inv_cell_of(nd):
    """1 / cell size for the largest neighbor_dist `nd`"""
    return 1.0 / (math.sqrt(nd * nd + 1.0e-5) * (1.0 + 1.0e-9))


def cell_of(x, inv_cell):
    return np.floor(np.asarray(x, np.float64) * inv_cell).astype(np.int64)


def first_double_of_cell(k, inv_cell):
    """the smallest double whose cell is k (its predecessor is the last one of cell k - 1): walked with nextafter under the model's own test"""
    x = np.float64(k / inv_cell)
    while cell_of(x, inv_cell) >= k:
        x = np.nextafter(x, -np.inf)
    while cell_of(x, inv_cell) < k:
        x = np.nextafter(x, np.inf)
    return float(x)


def equal_share_cells(pos, world, axis, inv_cell):
    """the cell cuts of sca_partition_init without cuts: equal shares of the agents as they stand, cells_sorted[r * n / world]"""
    cells = np.sort(cell_of(pos[:, axis], inv_cell))
    n = len(cells)
    return [int(cells[r * n // world]) for r in range(1, world)]


class Model:
    """who owns what: Model(world, axis, cuts, nd) from cut coordinates, or cell_cuts= the cuts in cells"""

    def __init__(self, world, axis, cuts=None, nd=10.0, cell_cuts=None):
        self.world, self.axis, self.inv_cell = int(world), int(axis), inv_cell_of(nd)
        if cell_cuts is None:
            cell_cuts = [int(math.floor(c * self.inv_cell)) for c in cuts]
        assert len(cell_cuts) == self.world - 1
        self.cell_cut = [-FAR] + [int(k) for k in cell_cuts] + [FAR]

    def accepted(self):
        """sca_partition_init's check: every INTERIOR rank has at least two layers of cells"""
        return all(self.cell_cut[r + 1] - self.cell_cut[r] >= 2 for r in range(1, self.world - 1))

    def layers(self, r):
        return self.cell_cut[r + 1] - self.cell_cut[r]

    def cells(self, pos):
        return cell_of(pos[:, self.axis], self.inv_cell)

    def owner(self, pos):
        """the rank that owns every agent"""
        return np.searchsorted(np.array(self.cell_cut[1:-1], np.int64), self.cells(pos), side='right').astype(np.int64)

    def halo(self, pos, r):
        """the agents rank r holds a copy of: those in the layer below its slab and in the layer above, where a peer exists"""
        c = self.cells(pos)
        out = np.zeros(len(c), bool)
        if r > 0:
            out |= c == self.cell_cut[r] - 1
        if r + 1 < self.world:
            out |= c == self.cell_cut[r + 1]
        return out

    def edge(self, pos, r):
        """the agents in rank r's own layers next to a peer (what its neighbours hold copies of)"""
        c = self.cells(pos)
        out = np.zeros(len(c), bool)
        if r > 0:
            out |= c == self.cell_cut[r]
        if r + 1 < self.world:
            out |= c == self.cell_cut[r + 1] - 1
        return out

    def headers(self, r, pos_old, pos_new):
        """(n_halo, n_mig) of rank r's outgoing message per side (0 below, 1 above; None where there is no peer), from the positions before
        and after a step.  Finished agents are owned agents whose record does not move: they count like everybody else."""
        owned = self.owner(pos_old) == r
        co, cn = self.cells(pos_old), self.cells(pos_new)
        out = [None, None]
        if r > 0:
            lo = self.cell_cut[r]
            leaves = owned & (cn < lo)
            out[0] = (int((owned & ((co == lo) | (cn == lo) | leaves)).sum()), int(leaves.sum()))
        if r + 1 < self.world:
            hi = self.cell_cut[r + 1]
            leaves = owned & (cn >= hi)
            out[1] = (int((owned & ((co == hi - 1) | (cn == hi - 1) | leaves)).sum()), int(leaves.sum()))
        return out

    def caps_needed(self, positions):
        """the smallest (cap_halo, cap_mig) that hold every message of a run: positions = [before the first step, after it, ...]"""
        nh = nm = 1
        for a, b in zip(positions[:-1], positions[1:]):
            for r in range(self.world):
                for h in self.headers(r, a, b):
                    if h is not None:
                        nh, nm = max(nh, h[0]), max(nm, h[1])
        return nh, nm


class Ranks:
    """`world` contexts of one process as the ranks of one swarm, stepped in PartitionedStepper.run's order with the peers' buffers handed
    over directly.  tracker: the goal headings for device_tracker_enable (None: no tracker).  cuts=None: the library's own (equal shares).
    The first ScaError ends the run: nothing more is stepped (`dead`)."""

    def __init__(self, S, scene, world, axis, cuts, per_agent=None, cap_halo=0, cap_mig=0, tracker=None):
        import torch
        from test_gpu_form_fuzz import context_of
        self.S, self.world, self.n, self.dead = S, int(world), scene['n'], False
        self.sols, self.out = [], []
        try:
            for r in range(self.world):
                sol = context_of(S, scene, per_agent, perm=False)
                self.sols.append(sol)
                if tracker is not None:
                    sol.device_tracker_enable(tracker)
            for r, sol in enumerate(self.sols):
                sol.partition_init(r, self.world, axis, cuts if self.world > 1 else None, cap_halo, cap_mig)
            nbytes = self.sols[0].partition_message_bytes()
            assert all(sol.partition_message_bytes() == nbytes for sol in self.sols)
            self.out = [[torch.zeros(nbytes, dtype=torch.uint8, device='cuda') for _ in (0, 1)] for _ in self.sols]
            torch.cuda.synchronize()                                             # (the contexts run on streams of their own)
        except BaseException:
            self.dead = True
            self.close()
            raise

    def _ptr(self, r, side):
        return self.out[r][side].data_ptr() if 0 <= r < self.world else 0

    def step(self):
        """one step of every rank.  The synchronisations between the two phases are what makes reading a peer's buffer (and, in the next
        step, rewriting one's own) safe."""
        assert not self.dead, 'a rank reported an error: nothing more is stepped'
        S = self.S
        try:
            if self.world == 1:                                                  # nobody to talk to: the whole step inside the library
                self.sols[0].run_steps(1, S.NBR_GRID)
                self.sols[0].synchronize()
                return
            for r, sol in enumerate(self.sols):
                sol.step_begin(S.NBR_GRID)
                sol.partition_pack(self._ptr(r, 0), self._ptr(r, 1))
            for sol in self.sols:
                sol.synchronize()
            for r, sol in enumerate(self.sols):
                sol.partition_unpack(self._ptr(r - 1, 1), self._ptr(r + 1, 0))       # what the rank below sent up, what the rank above sent down
                sol.partition_commit()
                sol.step_end()
            for sol in self.sols:
                sol.synchronize()
        except S.ScaError:
            self.dead = True
            raise

    def set_state(self, state):
        """the complete state on every rank (sca_set_state under a standing partition: ownership follows from it again)"""
        for sol in self.sols:
            sol.set_state(state['pos'], state['vel'], state['heading'], state['flags'], state['total_dist'], state['step_num'])

    def headers(self):
        """per rank and side the four int32 of the outgoing message's header (None where there is no peer)"""
        return [[self.out[r][side][:4 * HEADER_INTS].cpu().numpy().view(np.int32).copy() if 0 <= r + 2 * side - 1 < self.world else None
                 for side in (0, 1)] for r in range(self.world)]

    def owned(self):
        return [np.sort(sol.partition_owned()) for sol in self.sols]

    def gather(self, getter, owned=None):
        """one array (or dict of arrays) of the whole swarm, every row taken from the rank that owns it"""
        owned = self.owned() if owned is None else owned
        parts = [getter(sol) for sol in self.sols]
        if isinstance(parts[0], dict):
            out = {k: np.array(v) for k, v in parts[0].items()}
            for p, own in zip(parts, owned):
                for k in out:
                    out[k][own] = p[k][own]
            return out
        out = np.array(parts[0])
        for p, own in zip(parts, owned):
            out[own] = p[own]
        return out

    def close(self):
        for sol in self.sols:
            sol.close()
        self.sols = []
