"""Every EC kernel instantiation the dispatcher can pick, driven through the
C ABI (lizec_ec_encode_batch, lizec_ec_plan_create / lizec_ec_plan_run,
lizec_ec_encode_batch_multi, lizec_ec_plan_create_multi) at chosen
coefficients, with canaries around every output part.

Reference: a GF(2^8) multiply table built here with plain numpy from the
polynomial 0x11D; dest[l] = XOR_j mul[c[l][j]][src[j]].  A CPU test checks
that reference against the oracle before either judges a kernel.

The matrix (all bit-exact, num_stripes = 3):
  dests    1..8 run ec_encode_kernel<D = dests>; 9, 12, 16, 17, 32 run several
           passes, the later ones with a nonzero dest_base
  srcs     1, 2, 3, 32: the source loop is unrolled by two, so these are
           remainder-only, no remainder, remainder, and a long loop
  part_len with T the tile of the last pass (16 KiB for D <= 4, 8 KiB for
           D >= 5): 16, 4096, 4096+16, T-16 (ragged path only), T, and
           T+16, 3T+4096+16 (full-tile path, then a ragged tail)
Coefficients are random bytes with 0, 1, 2, 0x80 and 0xFF at fixed positions
and one all-zero row.  A matrix with fewer than five entries outside its zero
row cannot hold all of that at once; such a cell runs several matrices, which
together do (coef_matrices).
"""
import ctypes

import numpy as np
import pytest

import oracle

torch = pytest.importorskip("torch")

gpu = pytest.mark.gpu

LIZEC_OK = 0
S = 3                   # stripes per cell
GUARD = 256             # canary bytes before and after every output part
FILL = 0xA5
SPECIALS = (0, 1, 2, 0x80, 0xFF)

DESTS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 16, 17, 32)
SRCS = (1, 2, 3, 32)
SRCS_MULTI = (1, 3, 32)
LEN_NAMES = ("16", "4096", "4096+16", "T-16", "T", "T+16", "3T+4096+16")


def last_pass_d(dests):
    """Width of the last pass: run_batch takes 8 destinations at a time."""
    return dests - 8 * ((dests - 1) // 8)


def tile_bytes(dests):
    """ec_chunks_for: 4 chunks of 4 KiB for D <= 4, 2 for D >= 5."""
    return 16384 if last_pass_d(dests) <= 4 else 8192


def part_len(dests, name):
    T = tile_bytes(dests)
    return {"16": 16, "4096": 4096, "4096+16": 4096 + 16, "T-16": T - 16,
            "T": T, "T+16": T + 16, "3T+4096+16": 3 * T + 4096 + 16}[name]


MAX_LEN = 3 * 16384 + 4096 + 16


# ---------------------------------------------------------------- reference

def build_mul():
    """mul[a][b] = a*b in GF(2^8) mod x^8+x^4+x^3+x^2+1 (0x11D): shift-and-add
    over the bits of b."""
    a = np.repeat(np.arange(256, dtype=np.uint16)[:, None], 256, axis=1)
    b = np.arange(256, dtype=np.uint16)[None, :]
    prod = np.zeros((256, 256), np.uint16)
    for bit in range(8):
        prod ^= np.where((b >> bit) & 1, a, 0).astype(np.uint16)
        a = a << 1
        a = np.where(a & 0x100, a ^ 0x11D, a).astype(np.uint16)
    return prod.astype(np.uint8)


MUL = build_mul()


def isal_tables(coef):
    """32-byte ISA-L tables, one per coefficient in row-major order:
    tbl[i] = c*i, tbl[16+i] = c*(i<<4)."""
    c = np.ascontiguousarray(coef, np.uint8).ravel()
    nib = np.arange(16)
    t = np.empty((c.size, 32), np.uint8)
    t[:, :16] = MUL[c][:, nib]
    t[:, 16:] = MUL[c][:, nib << 4]
    return np.ascontiguousarray(t.ravel())


def ref_encode(coef, src):
    """coef [dests, srcs], src [S, srcs, L] -> [S, dests, L]."""
    dests, srcs = coef.shape
    out = np.zeros((src.shape[0], dests, src.shape[2]), np.uint8)
    for l in range(dests):
        for j in range(srcs):
            out[:, l] ^= MUL[coef[l, j]][src[:, j]]
    return out


def coef_matrices(dests, srcs, seed, rot=0):
    """The coefficient matrices of one cell: random bytes, row 1 all zero
    (when there is a row 1), and SPECIALS (rotated by `rot`) at fixed,
    evenly spread positions outside that row.  Where fewer than five such
    positions exist the specials are dealt over several matrices, and a
    one-row cell gets a further all-zero matrix for its zero row."""
    rng = np.random.default_rng(seed)
    zero_row = 1 if dests >= 2 else None
    free = [(l, j) for l in range(dests) if l != zero_row
            for j in range(srcs)]
    specials = SPECIALS[rot:] + SPECIALS[:rot]
    per = min(len(free), len(specials))
    mats = []
    for first in range(0, len(specials), per):
        chunk = specials[first:first + per]
        c = rng.integers(0, 256, (dests, srcs), np.uint8)
        if zero_row is not None:
            c[zero_row] = 0
        for i, v in enumerate(chunk):
            c[free[(i * len(free)) // per]] = v
        mats.append(c)
    if zero_row is None:
        mats.append(np.zeros((dests, srcs), np.uint8))
    return mats


_pool = None


def source_pool():
    """One random [S, 32, MAX_LEN] array shared (read-only) by all cells."""
    global _pool
    if _pool is None:
        _pool = np.random.default_rng(20240).integers(
            0, 256, (S, 32, MAX_LEN), np.uint8)
        _pool.setflags(write=False)
    return _pool


def cell_sources(srcs, plen):
    return np.array(source_pool()[:, :srcs, :plen], order="C")   # a copy


# ------------------------------------------- CPU: the references must agree

def test_mul_table_matches_oracle():
    for a in range(256):
        for b in (0, 1, 2, 3, 0x1D, 0x53, 0x80, 0xCA, 0xFF):
            assert MUL[a, b] == oracle.gf_mul(a, b), (a, b)
            assert MUL[b, a] == MUL[a, b]


def test_reference_matches_oracle():
    """numpy tables == oracle.init_tables and numpy encode ==
    oracle.ec_encode_data, on matrices that hold every special value and a
    zero row."""
    rng = np.random.default_rng(7)
    for dests, srcs, L in ((5, 3, 1040), (1, 1, 16), (2, 32, 272)):
        src = rng.integers(0, 256, (2, srcs, L), np.uint8)
        for coef in coef_matrices(dests, srcs, 99):
            tbl = isal_tables(coef)
            assert np.array_equal(tbl, oracle.init_tables(coef))
            exp = ref_encode(coef, src)
            for s in range(src.shape[0]):
                out = [np.full(L, 0x77, np.uint8) for _ in range(dests)]
                oracle.ec_encode_data(
                    tbl, [np.ascontiguousarray(src[s, j]) for j in range(srcs)],
                    out)
                assert np.array_equal(np.stack(out), exp[s]), (dests, srcs, s)


def test_every_cell_holds_the_chosen_coefficients():
    for dests in DESTS:
        for srcs in SRCS:
            for rot in (0, 2):
                mats = coef_matrices(dests, srcs, 1, rot)
                rows = [l for l in range(dests) if dests < 2 or l != 1]
                placed = set()   # specials can only be seen outside row 1
                for c in mats:
                    placed.update(int(v) for v in c[rows].ravel())
                assert placed.issuperset(SPECIALS), (dests, srcs, rot)
                assert any((c == 0).all(axis=1).any() for c in mats)
                if len(rows) * srcs >= 5:
                    assert len(mats) == (1 if dests >= 2 else 2)


# ------------------------------------------------------------- GPU plumbing

u8p = ctypes.POINTER(ctypes.c_uint8)
u32p = ctypes.POINTER(ctypes.c_uint32)
u64p = ctypes.POINTER(ctypes.c_uint64)


@pytest.fixture(scope="module")
def abi():
    from lizardfs_amd import lib as L
    return L.lib(), L.engine(0)


def stream_arg():
    return ctypes.c_void_p(torch.cuda.current_stream(0).cuda_stream)


class Cell:
    """Device buffers of one launch: sources [S, srcs, plen] and an output
    arena in which every part has GUARD canary bytes on either side."""

    def __init__(self, dests, srcs, plen, skip=None):
        self.dests, self.srcs, self.plen = dests, srcs, plen
        self.src_np = cell_sources(srcs, plen)
        self.d_src = torch.from_numpy(self.src_np).cuda()
        self.slot = GUARD + plen + GUARD
        self.arena = torch.full((S * dests, self.slot), FILL,
                                dtype=torch.uint8, device="cuda")
        assert self.d_src.data_ptr() % 16 == 0
        assert self.arena.data_ptr() % 16 == 0 and self.slot % 16 == 0
        self.src_ptrs = (np.uint64(self.d_src.data_ptr()) +
                         np.arange(S * srcs, dtype=np.uint64) *
                         np.uint64(plen))
        self.dst_ptrs = (np.uint64(self.arena.data_ptr() + GUARD) +
                         np.arange(S * dests, dtype=np.uint64) *
                         np.uint64(self.slot))
        self.skip = skip          # (stripe, dest) passed as address 0
        if skip is not None:
            self.dst_ptrs[skip[0] * dests + skip[1]] = 0

    def refill(self, fill):
        self.arena.fill_(fill)

    def check(self, exp, fill, what):
        """exp [S, dests, plen].  The whole arena is compared: parts,
        canaries, and the fill of a skipped part."""
        torch.cuda.synchronize()
        got = self.arena.cpu().numpy()
        want = np.full_like(got, fill)
        want[:, GUARD:GUARD + self.plen] = exp.reshape(S * self.dests,
                                                       self.plen)
        if self.skip is not None:
            want[self.skip[0] * self.dests + self.skip[1]] = fill
        if not np.array_equal(got, want):
            rows, cols = np.nonzero(got != want)
            inside = (cols >= GUARD) & (cols < GUARD + self.plen)
            first = [(int(r) // self.dests, int(r) % self.dests,
                      int(c) - GUARD) for r, c in zip(rows[:6], cols[:6])]
            pytest.fail(f"{what}: {rows.size} bytes differ, "
                        f"{int((~inside).sum())} of them in the canaries; "
                        f"first (stripe, dest, offset): {first}")
        assert np.array_equal(self.d_src.cpu().numpy(), self.src_np), \
            f"{what}: the sources were modified"


def ptr(a, t):
    return a.ctypes.data_as(t)


def run_single(abi, cell, coef, plan_runs=0):
    """Batch call; with plan_runs, a plan run that many times instead,
    the arena refilled with 0xEE before every run."""
    lib, eng = abi
    tbl = isal_tables(coef)
    args = (eng, cell.plen, cell.srcs, cell.dests, ptr(tbl, u8p),
            ptr(cell.src_ptrs, u64p), ptr(cell.dst_ptrs, u64p), S)
    exp = ref_encode(coef, cell.src_np)
    if not plan_runs:
        assert lib.lizec_ec_encode_batch(*args, stream_arg()) == LIZEC_OK
        cell.check(exp, FILL, "batch")
        return
    plan = ctypes.c_void_p()
    assert lib.lizec_ec_plan_create(*args, ctypes.byref(plan)) == LIZEC_OK
    try:
        for run in range(plan_runs):
            cell.refill(0xEE)
            assert lib.lizec_ec_plan_run(plan, stream_arg()) == LIZEC_OK
            cell.check(exp, 0xEE, f"plan run {run}")
    finally:
        torch.cuda.synchronize()
        lib.lizec_ec_plan_destroy(plan)


def run_multi(abi, cell, coefs, plan_runs=0):
    """Two tables, tbl_index alternating per stripe."""
    lib, eng = abi
    tbl = np.concatenate([isal_tables(c) for c in coefs])
    index = (np.arange(S) % len(coefs)).astype(np.uint32)
    args = (eng, cell.plen, cell.srcs, cell.dests, ptr(tbl, u8p), len(coefs),
            ptr(index, u32p), ptr(cell.src_ptrs, u64p),
            ptr(cell.dst_ptrs, u64p), S)
    exp = np.concatenate([ref_encode(coefs[index[s]], cell.src_np[s:s + 1])
                          for s in range(S)])
    if not plan_runs:
        assert lib.lizec_ec_encode_batch_multi(*args, stream_arg()) == LIZEC_OK
        cell.check(exp, FILL, "multi batch")
        return
    plan = ctypes.c_void_p()
    assert lib.lizec_ec_plan_create_multi(*args,
                                          ctypes.byref(plan)) == LIZEC_OK
    try:
        for run in range(plan_runs):
            cell.refill(0xEE)
            assert lib.lizec_ec_plan_run(plan, stream_arg()) == LIZEC_OK
            cell.check(exp, 0xEE, f"multi plan run {run}")
    finally:
        torch.cuda.synchronize()
        lib.lizec_ec_plan_destroy(plan)


def cell_seed(dests, srcs, lname):
    return 1000 * dests + 10 * srcs + LEN_NAMES.index(lname)


# ------------------------------------------------------------------- matrix

@gpu
@pytest.mark.parametrize("lname", LEN_NAMES)
@pytest.mark.parametrize("srcs", SRCS)
@pytest.mark.parametrize("dests", DESTS)
def test_single_table(abi, dests, srcs, lname):
    plen = part_len(dests, lname)
    for coef in coef_matrices(dests, srcs, cell_seed(dests, srcs, lname)):
        run_single(abi, Cell(dests, srcs, plen), coef)


@gpu
@pytest.mark.parametrize("lname", LEN_NAMES)
@pytest.mark.parametrize("srcs", SRCS_MULTI)
@pytest.mark.parametrize("dests", DESTS)
def test_multi_table(abi, dests, srcs, lname):
    """Stripes 0 and 2 use table 0, stripe 1 table 1; stripe 1's middle
    destination has address 0 and must keep its fill.  The lengths T, T+16
    and 3T+4096+16 are the full-tile cells, for every D including 5..8."""
    plen = part_len(dests, lname)
    seed = cell_seed(dests, srcs, lname)
    a = coef_matrices(dests, srcs, seed)
    b = coef_matrices(dests, srcs, seed + 500000, rot=2)
    for c0, c1 in zip(a, b):
        assert not np.array_equal(c0, c1) or not c0.any()
        run_multi(abi, Cell(dests, srcs, plen, skip=(1, dests // 2)),
                  (c0, c1))


@gpu
@pytest.mark.parametrize("lname", ("T", "T+16"))
@pytest.mark.parametrize("dests", (3, 7, 9))
@pytest.mark.parametrize("form", ("single", "multi"))
def test_plan_runs_equal_batch(abi, form, dests, lname):
    """A plan run twice, the outputs refilled with 0xEE in between, gives
    what the batch call gives (both are held to the same reference)."""
    srcs = 3
    plen = part_len(dests, lname)
    seed = cell_seed(dests, srcs, lname) + 7
    if form == "single":
        coef = coef_matrices(dests, srcs, seed)[0]
        run_single(abi, Cell(dests, srcs, plen), coef)
        run_single(abi, Cell(dests, srcs, plen), coef, plan_runs=2)
    else:
        coefs = (coef_matrices(dests, srcs, seed)[0],
                 coef_matrices(dests, srcs, seed + 500000, rot=2)[0])
        skip = (1, dests // 2)
        run_multi(abi, Cell(dests, srcs, plen, skip=skip), coefs)
        run_multi(abi, Cell(dests, srcs, plen, skip=skip), coefs,
                  plan_runs=2)


@gpu
def test_single_table_grid_stride(abi):
    """part_len 16, three stripes more than the grid cap of 1,048,576
    blocks: the smallest shape at which a block of ec_encode_kernel runs a
    second tile.  Every stripe has its own source and destination rows."""
    lib, eng = abi
    srcs, dests, plen = 3, 2, 16
    n = 1048576 + 3
    rng = np.random.default_rng(31)
    src_np = rng.integers(0, 256, (n, srcs, plen), np.uint8)
    coef = np.array([[0x80, 1, 0xFF], [2, 0x1D, 0x53]], np.uint8)
    d_src = torch.from_numpy(src_np).cuda()
    d_out = torch.full((n, dests, plen), FILL, dtype=torch.uint8,
                       device="cuda")
    src_ptrs = (np.uint64(d_src.data_ptr()) +
                np.arange(n * srcs, dtype=np.uint64) * np.uint64(plen))
    dst_ptrs = (np.uint64(d_out.data_ptr()) +
                np.arange(n * dests, dtype=np.uint64) * np.uint64(plen))
    tbl = isal_tables(coef)
    assert lib.lizec_ec_encode_batch(
        eng, plen, srcs, dests, ptr(tbl, u8p), ptr(src_ptrs, u64p),
        ptr(dst_ptrs, u64p), n, stream_arg()) == LIZEC_OK
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    exp = ref_encode(coef, src_np)
    bad = np.flatnonzero((got != exp).any(axis=(1, 2)))
    assert bad.size == 0, f"{bad.size} stripes differ, first {bad[:8]}"
    assert np.array_equal(d_src.cpu().numpy(), src_np)
