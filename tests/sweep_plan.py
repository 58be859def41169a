"""A Python twin of the host dispatch of the product sweeps: given (M, N, dtype, CU count, csmp_tune overrides) it returns what the
host would launch, as kernel names with their template arguments, and where each sweep body puts a column (workgroup, wave, position
in the wave's sequence).  No GPU, no import of the library: tests/test_sweep_plan_static.py checks the twin against the documented
choices and the built kernel list, tests/test_gpu_sweep_matrix.py asserts sweep_config() against it before every launch and uses the
column maps to plant ties.  Every rule cites the line it mirrors (csrc/ = compressedsensing.jl_amd/csrc/)."""
from dataclasses import dataclass, field

K_WAVE = 64           # csmp_kernels.hpp:23
SWEEP_THREADS = 256   # csmp_kernels.hpp:24
NW = SWEEP_THREADS // K_WAVE
MULTI_THREADS = 512   # csmp_kernels.hpp:2116
GROUP_MAX = 4         # csmp_kernels.hpp:2114
WIDE_MAX = 2 * GROUP_MAX
CLAIM_MAX_WGS = 512   # csmp_kernels.hpp:883
PAIR_TICK_GRID = 192  # host/ctx.hpp:173
GROUP_TICK_GRID = 208  # host/ctx.hpp:174
WIDE_TICK_GRID = 256  # host/ctx.hpp:175
PAIR_MIN_BYTES = 4 << 20  # host/batch_io.hpp:141
LDS_CAP = 160 * 1024 - 512  # host/dictionary.hpp:151


def _f32(dtype):
    import numpy as np
    dt = np.dtype(dtype)
    assert dt in (np.dtype(np.float32), np.dtype(np.float64))
    return dt == np.dtype(np.float32)


def sweep_gen_lds_bytes(KP):  # csmp_kernels.hpp:462
    return (KP + 8 + 16 + 8) * 8


def sweep_ph_lds_bytes(KP, pcap):  # csmp_kernels.hpp:479
    return (KP + 8 + 16 + 8 + 8 + 4 * pcap) * 8


def sweep_dyn_lds_bytes(KP):  # csmp_kernels.hpp:887
    return (KP + 8 + 16 + 8 + 16) * 8


def sweep_multi_lds_bytes(KP, R):  # csmp_kernels.hpp:2126-2129
    nred = R * 4 * (MULTI_THREADS // K_WAVE)
    return (R * KP + 16 + nred) * 8 + nred * 4


def fr_sweep_lds_bytes(Mv, vec, U, nq):  # csmp_forward.hpp:235-241
    rows = K_WAVE * vec
    nchunk = (Mv + rows - 1) // rows
    nblocks = (nchunk + U - 1) // U
    images = 4 if nq == 4 else 1 + (nq if nq > 0 else 0)
    return (images * nblocks * U * rows + 8 + 16 + 8) * 8


def balanced_grid(N, base):  # host/dictionary.hpp:121-137
    groups = (N + NW - 1) // NW
    if groups <= base:
        return max(1, groups)
    grid = base
    if N // (4 * base) < 32:
        best = 0.0
        for g in range(base + base // 8, base - base // 8 - 1, -1):
            per_wave = (N + 4 * g - 1) // (4 * g)
            eff = N / (per_wave * 4 * g)
            if eff > best + 5e-3:
                best, grid = eff, g
    return int(grid)


@dataclass
class Plan:
    """ctx's fields after configure_sweep (host/dictionary.hpp:146-230), by their names there"""
    M: int
    N: int
    f32: bool
    cus: int
    tunes: dict = field(default_factory=dict)
    vec: int = 0
    rows: int = 0
    Mv: int = 0
    nchunk: int = 0
    sweep_U: int = 0
    sweep_KP: int = 0
    sweep_ph: bool = False
    sweep_pcap: int = 0
    sweep_dyn: bool = False
    sweep_grid: int = 0
    tick_grid: int = 0
    sweep_lds: int = 0
    sweep_group: int = 0
    group_wide: int = 0
    short_nch: int = 0
    short_cpu: int = 0
    short_KP: int = 0

    def tune(self, key):
        return int(self.tunes.get(key, 0))

    # ---- what csmp_sweep_config reports (host/measure.hpp:209-236)
    def config(self):
        return {"unit_loads": self.sweep_U,
                "phases": (self.Mv + self.sweep_KP - 1) // self.sweep_KP if self.sweep_ph else 1,  # :213
                "workgroups": self.sweep_grid,
                "tick_workgroups": self.tune("tick_grid") if self.tune("tick_grid") > 0 else self.tick_grid,  # :215
                "lds_bytes": self.sweep_lds,
                "dynamic": 1 if self.sweep_dyn else 0,
                "columns_per_unit": 8 // self.short_nch if self.short_cpu > 0 else 1,  # :218
                "group_max": self.sweep_group, "group_wide": self.group_wide}

    @property
    def ta(self):
        return "float" if self.f32 else "double"

    # ---- sweep_product (host/dictionary.hpp:63-81); ncols > 0: a sweep over the first columns only (never dynamic, :68)
    def sweep(self, ncols=0):
        if self.short_cpu > 0 and self.short_nch == 1:  # :65
            return ("k_sweep_short", self.ta, 1, 4)
        if self.short_cpu > 0 and self.short_nch == 2:  # :66
            return ("k_sweep_short", self.ta, 2, 4)
        if self.short_cpu > 0:  # :67
            return ("k_sweep_short", self.ta, 4, 2)
        u = self.sweep_U if self.sweep_U in (16, 8) else 4  # the switches' default arm, :72 / :79
        if self.sweep_dyn and ncols == 0:  # :68-74
            return ("k_sweep_dyn", self.ta, u, 32 // u)
        if self.sweep_ph:  # :75, sweep_launch_ph :44
            return ("k_sweep_ph", self.ta, 8, 4)
        return ("k_sweep_gen", self.ta, u, 32 // u)  # :76-80

    # ---- tick_launch (host/omp.hpp:53-68): k_tick<TA, U, PH, STEADY, DYN>
    def tick(self, steady):
        if self.sweep_ph:  # :55
            return ("k_tick", self.ta, 8, True, bool(steady), False)
        u = self.sweep_U if self.sweep_U in (16, 8) else 4
        return ("k_tick", self.ta, u, False, bool(steady), bool(self.sweep_dyn))  # :56-67

    def pipe_nblk(self, grid):  # host/omp.hpp:96-100
        groups = (self.N + NW - 1) // NW
        g = self.tune("tick_grid") if self.tune("tick_grid") > 0 else grid
        return max(1, min(min(g, groups), self.cus * 8 + 8))

    def wide_nblk(self):  # host/omp.hpp:102
        return max(16, self.pipe_nblk(WIDE_TICK_GRID) // 16 * 16)

    def shared_nblk(self):  # host/mp_batch.hpp:103, host/forward.hpp:299 (Grouped)
        return self.pipe_nblk(GROUP_TICK_GRID if self.f32 else PAIR_TICK_GRID)

    def two_pipelines(self):  # host/batch_io.hpp:138-144
        p = self.tune("pipelines")
        return p != 1 and (p >= 2 or self.Mv * self.N * (4 if self.f32 else 8) >= PAIR_MIN_BYTES)

    # ---- shared_pass_launch / multi_launch / wide_launch (host/omp.hpp:153-252)
    def shared(self, size):
        """the pass of a group of `size` members: (kernel, TA, U, R[, NT]) and the number of column streams"""
        assert self.sweep_group >= 1 and 1 <= size <= max(self.group_wide, self.sweep_group)
        if size > GROUP_MAX:  # :242, multi_members :211-213, wide_launch_nt :192-198, kWideNt :201
            assert self.f32
            return ("k_sweep_wide", "float", 4, (size + 1) // 2, False), self.wide_nblk() // 2
        if self.f32:  # :158, :231
            return ("k_sweep_multi", "float", 4, size), self.shared_nblk()
        u = self.sweep_U if self.sweep_U in (16, 8) else 4  # :224-229
        return ("k_sweep_multi_w4", "double", u, size), self.shared_nblk()

    # ---- fr_config / fr_tall (host/forward.hpp:49-84)
    def fr_config(self, nq):
        U, full = 4, False
        if self.Mv % self.rows == 0:  # :54
            nchunk = self.Mv // self.rows
            tu = self.tune("sweep_unit")
            umax = 16 if tu == 16 else 8 if tu == 8 else 16 if nq == 2 else 8  # :62
            for u in (16, 8):  # :63-68
                if u <= umax and nchunk % u == 0:
                    U, full = u, True
                    break
        lds = fr_sweep_lds_bytes(self.Mv, self.vec, U, nq)  # :70
        g = self.cus * (15 if nq == 2 else 12) // 16 if U == 16 else self.cus  # :72
        if self.tune("sweep_grid") > 0:  # :73
            g = min(self.tune("sweep_grid"), self.cus * 8)
        groups = (self.N + NW - 1) // NW
        return U, full, lds, max(1, min(g, groups))  # :75

    def fr_tall(self, nq):  # :80-84
        return self.fr_config(nq)[2] > LDS_CAP

    def fr_pass(self, nq):
        """launch_fr_pass (host/forward.hpp:144-156): 'tall' (separate product sweeps + k_fr_combine) or k_fr_sweep<TA, U, FULL, NQ>"""
        if self.fr_tall(nq):  # :145
            return "tall"
        U, full, _, _ = self.fr_config(nq)
        if not full:  # fr_sweep_launch :42
            return ("k_fr_sweep", self.ta, 4, False, nq)
        return ("k_fr_sweep", self.ta, 16 if U == 16 else 8, True, nq)  # :43-44

    def fr_tick(self, first):
        """fr_pipe_launch (host/forward.hpp:202-203) where batch_schedule takes the tick (:252-256), else None: one signal at a time"""
        U, full, _, _ = self.fr_config(1)
        if not full or self.fr_tall(1):  # :255
            return None
        return ("k_tick_fr", self.ta, 16 if U == 16 else 8, -1 if first else 1)


def plan(M, N, dtype, cus, tunes=None):
    """configure_sweep (host/dictionary.hpp:146-230) for a dictionary copied from the host (Mv = M padded to 16 bytes, :328-335)"""
    p = Plan(int(M), int(N), _f32(dtype), int(cus), dict(tunes or {}))
    p.vec = 4 if p.f32 else 2  # :147
    p.rows = K_WAVE * p.vec  # :148
    p.Mv = (p.M + p.vec - 1) // p.vec * p.vec
    p.nchunk = nchunk = (p.Mv + p.rows - 1) // p.rows  # :149
    kp_cap = LDS_CAP // 8 - 48  # :152
    bestU = best_pad = 0
    for u in (16, 8, 4):  # :155-163
        if p.tune("sweep_unit") > 0 and u != p.tune("sweep_unit"):
            continue
        pad = (nchunk + u - 1) // u * u
        if pad * p.rows > kp_cap:
            continue
        if not bestU or pad < best_pad:
            bestU, best_pad = u, pad
    col_bytes = p.Mv * (4 if p.f32 else 8)  # :164
    base = p.cus * 3 // 4 if col_bytes >= 8192 else p.cus * 3  # :165
    maxgrid = p.cus * 8 + 8  # :166
    tg = p.tune("sweep_grid")
    p.sweep_grid = balanced_grid(p.N, tg if tg > 0 else base)  # :167
    if tg > 0 and tg < p.sweep_grid + p.sweep_grid // 4:  # :168-171
        p.sweep_grid = max(1, min(tg, (p.N + 3) // 4))
    p.tick_grid = balanced_grid(p.N, p.cus * 11 // 16 if col_bytes >= 8192 else p.cus * 3)  # :173
    p.sweep_grid = min(p.sweep_grid, maxgrid)  # :174
    p.tick_grid = min(p.tick_grid, maxgrid)  # :175
    tick_nblk = p.tune("tick_grid")
    if bestU:  # :177-179
        p.sweep_U, p.sweep_KP = bestU, best_pad * p.rows
    else:  # :180-197
        ming = min(p.sweep_grid, tick_nblk if tick_nblk > 0 else min(p.tick_grid, PAIR_TICK_GRID))
        pcap = (p.N + ming * 4 - 1) // (ming * 4)
        spare = LDS_CAP // 8 - 48 - 4 * pcap
        ur = 8 * p.rows
        if spare < ur:
            raise ValueError("too many columns per sweep workgroup for a residual staged in phases")  # :188
        p.sweep_pcap = pcap
        kp_max = spare // ur * ur
        if p.tune("phase_rows") > 0:  # :191
            kp_max = max(ur, min(kp_max, p.tune("phase_rows") // ur * ur))
        nph = (p.Mv + kp_max - 1) // kp_max
        per = (p.Mv + nph - 1) // nph
        p.sweep_U, p.sweep_ph, p.sweep_KP = 8, True, (per + ur - 1) // ur * ur
    p.sweep_dyn = (not p.sweep_ph) and p.tune("sweep_dyn") >= 1  # :199
    if p.sweep_grid > CLAIM_MAX_WGS or max(p.tick_grid, tick_nblk) > CLAIM_MAX_WGS:  # :200
        p.sweep_dyn = False
    p.sweep_lds = (sweep_ph_lds_bytes(p.sweep_KP, p.sweep_pcap) if p.sweep_ph else
                   sweep_dyn_lds_bytes(p.sweep_KP) if p.sweep_dyn else sweep_gen_lds_bytes(p.sweep_KP))  # :201-202
    p.sweep_group = 0  # :207-213
    if not p.sweep_ph and not p.sweep_dyn:
        g = GROUP_MAX
        while g > 1 and sweep_multi_lds_bytes(p.sweep_KP, g) > LDS_CAP:
            g -= 1
        if p.tune("group_max") > 0:
            g = min(g, p.tune("group_max"))
        p.sweep_group = g
    p.group_wide = (WIDE_MAX if p.sweep_group == GROUP_MAX and p.f32 and p.tune("group_wide") != 1 and p.tune("group_max") == 0
                    else p.sweep_group)  # :217-218
    if p.tune("sweep_short") != 1 and nchunk <= 4 and p.N >= 8:  # :223-228
        p.short_nch = nchunk if nchunk <= 2 else 4
        p.short_cpu = 4 if nchunk <= 2 else 2
        p.short_KP = p.short_nch * p.rows
    return p


# ------------------------------------------------------------------------------------------ where a body puts a column
# Every static body deals the columns (or column pairs, or column groups) round-robin over the grid's waves and a wave takes its own
# in increasing order; a wave's c values leave in stores of `store` columns plus the final flush.
def column_owner(body, col, nblk, nch=0):
    """(workgroup, wave, position in the wave's column sequence, columns per wave store) of column `col` on a grid of nblk column streams.
    gen / ph / multi_w4: col0 = bid * NW + wave, stride nblk * NW, one column at a time, CStage stores 64 columns
        (csmp_kernels.hpp:344, :502, :2394; CStage :282-285, :301).
    multi (also a stream of k_sweep_wide, nblk = streams): PAIRS q = bid * 8 + wave + i * nblk * 8 of the columns 2q, 2q + 1, two
        CStage slots per pair (:2158, :2318-2320).
    short: GROUPS of 8 / NCH neighbouring columns, g0 = bid * NW + wave, stride nblk * NW; 64 * KS = 384 columns per store (:702, :709).
    dyn: the columns are claimed at run time (:893 ff.) -- no static map."""
    if body in ("gen", "ph", "multi_w4"):
        w = col % (nblk * NW)
        return w // NW, w % NW, col // (nblk * NW), 64
    if body == "multi":
        nw = MULTI_THREADS // K_WAVE
        q = col // 2
        w = q % (nblk * nw)
        return w // nw, w % nw, 2 * (q // (nblk * nw)) + col % 2, 64
    if body == "short":
        cu = 8 // nch
        g = col // cu
        w = g % (nblk * NW)
        return w // NW, w % NW, cu * (g // (nblk * NW)) + col % cu, 384
    raise ValueError(body)


def wave_columns(body, bid, wave, N, nblk, nch=0):
    """the columns wave `wave` of workgroup (column stream) `bid` owns, in the order it finishes them"""
    if body in ("gen", "ph", "multi_w4"):
        return list(range(bid * NW + wave, N, nblk * NW))
    if body == "multi":
        nw = MULTI_THREADS // K_WAVE
        out = []
        for q in range(bid * nw + wave, (N + 1) // 2, nblk * nw):
            out += [c for c in (2 * q, 2 * q + 1) if c < N]
        return out
    if body == "short":
        cu = 8 // nch
        out = []
        for g in range(bid * NW + wave, (N + cu - 1) // cu, nblk * NW):
            out += [c for c in range(g * cu, g * cu + cu) if c < N]
        return out
    raise ValueError(body)


def body_of(kernel):
    """the column map a kernel of a plan uses"""
    name = kernel[0]
    if name == "k_sweep_short":
        return "short"
    if name in ("k_sweep_multi", "k_sweep_wide"):
        return "multi"
    if name == "k_sweep_multi_w4":
        return "multi_w4"
    if name == "k_sweep_dyn" or (name == "k_tick" and kernel[5]):
        return "dyn"
    if name == "k_sweep_ph" or (name == "k_tick" and kernel[3]):
        return "ph"
    return "gen"


def chain_length(p, kernel):
    """n of the bound gamma_n sum|a r|: the fmas of one lane's chain over a column plus the six additions of the butterfly (wave_xsum,
    csmp_kernels.hpp:125).  gen / dyn / multi / multi_w4 / tick: one chain over the KP / 64 rows a lane holds of the image (:399-415,
    :2162 'every row of the image', :2451 ff., :1030 ff.).  short: NCH chunks (:757-772).  ph: a chain per stage and one addition per
    further stage to join the stages' partial sums (:600-640)."""
    body = body_of(kernel)
    if body == "short":
        return p.short_nch * p.vec + 6
    if body == "ph":
        nph = (p.Mv + p.sweep_KP - 1) // p.sweep_KP
        return p.sweep_KP // K_WAVE + (nph - 1) + 6
    return p.sweep_KP // K_WAVE + 6


def kernel_name(k):
    """the demangled name as the code object lists it, e.g. 'k_sweep_gen<float, 16, 2>'"""
    return k[0] + "<" + ", ".join(("true" if a else "false") if isinstance(a, bool) else str(a) for a in k[1:]) + ">"
