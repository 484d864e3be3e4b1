"""Every CRC kernel lizec_crc32_batch can pick, and its input edges, against
oracle.crc32_blocks and (as a second, independent reference) zlib.crc32.

  large blocks   the combine tree appends zero runs of up to block_len / 2
                 bytes with the matrices M_0..M_25; blocks of 2^26 and just
                 under 2^27 bytes use M_20..M_25, 2^27 is refused
  burst counts   the prefetch shape folds two 8 KiB-per-wave bursts per
                 iteration; 8..40 KiB blocks are 1..5 bursts (2..10 at BV=4)
  variants       every kernel an environment hook selects, at the smallest
                 block its divisibility rule admits and at 64 KiB
  alignment      buffers at 4 and 8 bytes off a 16-byte boundary take the
                 dword-load kernels at every block length; 1 off is refused
  grid stride    more than 524,288 blocks make every wave loop
"""
import ctypes
import os
import zlib

import numpy as np
import pytest

import oracle

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

LIZEC_OK = 0
LIZEC_EINVAL = -2
SEEDS = (0, 0xABCD1234)
ENV_KEYS = ("LIZEC_CRC_AUTOTUNE", "LIZEC_CRC_PF", "LIZEC_CRC_BV",
            "LIZEC_CRC_CHAINS", "LIZEC_CRC_FOLD_NACC", "LIZEC_CRC_NT",
            "LIZEC_CRC_IMPL", "LIZEC_CRC_SLICE")


@pytest.fixture(scope="module")
def crc_mod():
    from lizardfs_amd import crc
    return crc


class crc_env:
    """Set the dispatch hooks for one case (autotuning always off); every
    variable is restored on exit."""

    def __init__(self, **env):
        self.env = dict({"LIZEC_CRC_AUTOTUNE": "0"},
                        **{"LIZEC_CRC_" + k: str(v) for k, v in env.items()})
        assert set(self.env) <= set(ENV_KEYS)

    def __enter__(self):
        self.saved = {k: os.environ.get(k) for k in ENV_KEYS}
        for k in ENV_KEYS:
            os.environ.pop(k, None)
        os.environ.update(self.env)
        return self

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        return False


def device_random(nbytes, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device="cuda",
                         generator=g)


def gpu_crcs(crc_mod, buf, block_len, seed):
    got = crc_mod.crc32_blocks(buf, block_len, seed=seed)
    torch.cuda.synchronize()
    return got.cpu().numpy().view(np.uint32)


def zlib_blocks(host, block_len, seed):
    mv = memoryview(host)
    return np.array([zlib.crc32(mv[o:o + block_len], seed)
                     for o in range(0, host.size, block_len)], np.uint32)


def check_blocks(crc_mod, buf, host, block_len, what, use_zlib=True):
    for seed in SEEDS:
        exp = oracle.crc32_blocks(host, block_len, seed=seed)
        if use_zlib:
            assert np.array_equal(exp, zlib_blocks(host, block_len, seed)), \
                f"{what}: the two references disagree"
        got = gpu_crcs(crc_mod, buf, block_len, seed)
        bad = np.flatnonzero(got != exp)
        assert bad.size == 0, \
            f"{what} seed {seed:#x}: {bad.size} of {exp.size} blocks " \
            f"differ, first {bad[:8]}"


# ------------------------------------------------------------ large blocks

@pytest.mark.parametrize("block_len,nblocks", [
    (1 << 26, 1),
    (1 << 26, 2),
    ((1 << 26) - 8192, 1),
    ((1 << 27) - 8192, 1),          # the longest fold-eligible block
    ((1 << 26) - 1024, 1),          # not a multiple of 8 KiB: generic kernel
    ((1 << 27) - 1024, 1),          # the longest block of all
], ids=["2^26", "2^26x2", "2^26-8192", "2^27-8192", "2^26-1024",
        "2^27-1024"])
def test_large_blocks(crc_mod, block_len, nblocks):
    buf = device_random(block_len * nblocks, 100 + nblocks)
    host = buf.cpu().numpy()
    with crc_env():
        check_blocks(crc_mod, buf, host, block_len, f"block_len {block_len}")
    if block_len % 16384 == 0:
        # the same length through a slicing kernel's combine tree
        with crc_env(IMPL="table"):
            check_blocks(crc_mod, buf, host, block_len,
                         f"block_len {block_len} table", use_zlib=False)


def test_block_length_bound(crc_mod):
    """block_len = 2^27 would index past the matrix bank: LIZEC_EINVAL from
    the host, the output untouched; the wrapper raises ValueError."""
    from lizardfs_amd import lib as L
    block_len = 1 << 27
    buf = torch.zeros(block_len + 1024, dtype=torch.uint8, device="cuda")
    out = torch.full((4,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream(0).cuda_stream)
    for bl in (block_len, block_len + 1024):
        rc = L.lib().lizec_crc32_batch(
            L.engine(0), ctypes.c_void_p(buf.data_ptr()), bl, 1, 0,
            ctypes.c_void_p(out.data_ptr()), stream)
        assert rc == LIZEC_EINVAL, bl
    torch.cuda.synchronize()
    assert bool((out == 0x5A5A5A5A).all()), "a refused call wrote its output"
    with pytest.raises(ValueError, match="block_len"):
        crc_mod.crc32_blocks(buf[:block_len], block_len)


# ------------------------------------------------------------ burst counts

@pytest.mark.parametrize("env", [{}, {"BV": 4}, {"PF": 1},
                                 {"PF": 1, "BV": 4}],
                         ids=["default", "BV4", "PF", "PF-BV4"])
@pytest.mark.parametrize("block_len", [8192, 16384, 24576, 32768, 40960])
def test_burst_counts(crc_mod, block_len, env):
    buf = device_random(8 * block_len, block_len)
    host = buf.cpu().numpy()
    with crc_env(**env):
        check_blocks(crc_mod, buf, host, block_len, f"{block_len} {env}")


# ---------------------------------------------------------------- variants

VARIANTS = [
    # (environment, smallest admissible block)
    ({"CHAINS": 2, "FOLD_NACC": 1}, 16384),
    ({"CHAINS": 2, "FOLD_NACC": 2}, 16384),
    ({"FOLD_NACC": 2}, 8192),
    ({"FOLD_NACC": 2, "BV": 4}, 8192),
    ({"FOLD_NACC": 4}, 8192),
    ({"FOLD_NACC": 4, "BV": 4}, 8192),
    ({"NT": 1, "FOLD_NACC": 1}, 8192),
    ({"NT": 1, "FOLD_NACC": 2}, 8192),
    ({"NT": 1, "FOLD_NACC": 4}, 8192),
    ({"IMPL": "table", "SLICE": 8}, 16384),
    ({"IMPL": "table", "SLICE": 16}, 16384),
    ({"IMPL": "table", "CHAINS": 4}, 32768),
]


def variant_id(v):
    return "-".join(f"{k}{x}" for k, x in v[0].items())


@pytest.mark.parametrize("variant", VARIANTS, ids=variant_id)
def test_env_variants(crc_mod, variant):
    env, smallest = variant
    for block_len in (smallest, 65536):
        buf = device_random(8 * block_len, 7 + block_len)
        host = buf.cpu().numpy()
        with crc_env(**env):
            check_blocks(crc_mod, buf, host, block_len,
                         f"{env} block_len {block_len}")


# --------------------------------------------------------------- alignment

@pytest.mark.parametrize("env", [{}, {"CHAINS": 2}, {"IMPL": "table"},
                                 {"CHAINS": 4}],
                         ids=["default", "CHAINS2", "table", "CHAINS4"])
@pytest.mark.parametrize("block_len", [65536, 16384, 8192, 1024, 3072])
@pytest.mark.parametrize("offset", [4, 8])
def test_unaligned_buffer(crc_mod, offset, block_len, env):
    """4- and 8-byte aligned buffers are read with dword loads: by the fold
    kernels' AL16=false forms at multiples of 8 KiB (one chain, or two under
    CHAINS=2 at multiples of 16 KiB), by the generic kernel's otherwise,
    whatever the hooks ask for."""
    big = device_random(8 * block_len + 64, offset + block_len)
    assert big.data_ptr() % 16 == 0
    buf = big[offset:offset + 8 * block_len]
    assert buf.data_ptr() % 16 == offset and buf.is_contiguous()
    host = buf.cpu().numpy()
    with crc_env(**env):
        check_blocks(crc_mod, buf, host, block_len,
                     f"offset {offset} block_len {block_len} {env}")


@pytest.mark.parametrize("block_len", [65536, 1024])
@pytest.mark.parametrize("offset", [1, 2, 7])
def test_misaligned_buffer_refused(crc_mod, offset, block_len):
    """A buffer that is not 4-byte aligned is refused on the host: no kernel
    has loads that are legal there."""
    from lizardfs_amd import lib as L
    big = torch.zeros(2 * block_len + 64, dtype=torch.uint8, device="cuda")
    buf = big[offset:offset + 2 * block_len]
    out = torch.full((2,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    rc = L.lib().lizec_crc32_batch(
        L.engine(0), ctypes.c_void_p(buf.data_ptr()), block_len, 2, 0,
        ctypes.c_void_p(out.data_ptr()),
        ctypes.c_void_p(torch.cuda.current_stream(0).cuda_stream))
    assert rc == LIZEC_EINVAL
    torch.cuda.synchronize()
    assert bool((out == 0x5A5A5A5A).all()), "a refused call wrote its output"
    with pytest.raises(ValueError, match="aligned"):
        crc_mod.crc32_blocks(buf, block_len)


# ------------------------------------------------------------- grid stride

PERIOD = 4099   # prime: no stride of a wave's loop is a multiple of it


@pytest.mark.parametrize("block_len,envs", [
    (8192, ({}, {"PF": 1})),    # fold path, 4 GiB
    (1024, ({},)),              # generic kernel, 512 MiB
], ids=["fold-8192", "generic-1024"])
def test_grid_stride(crc_mod, block_len, envs):
    """524,288 + 5 blocks: five waves run a second block.  The buffer
    repeats a random pattern of 4099 blocks, so block b must carry the CRC
    of pattern block b % 4099."""
    nblocks = 524288 + 5
    pat = device_random(PERIOD * block_len, block_len)
    host = pat.cpu().numpy()
    buf = torch.empty(nblocks * block_len, dtype=torch.uint8, device="cuda")
    reps = nblocks // PERIOD
    whole = reps * PERIOD * block_len
    buf[:whole].view(reps, PERIOD * block_len).copy_(
        pat.unsqueeze(0).expand(reps, -1))
    buf[whole:].copy_(pat[:buf.numel() - whole])
    which = np.arange(nblocks) % PERIOD
    refs = {}
    for seed in SEEDS:
        refs[seed] = oracle.crc32_blocks(host, block_len, seed=seed)
        assert np.array_equal(refs[seed], zlib_blocks(host, block_len, seed))
    for env in envs:
        with crc_env(**env):
            for seed in SEEDS:
                got = gpu_crcs(crc_mod, buf, block_len, seed)
                bad = np.flatnonzero(got != refs[seed][which])
                assert bad.size == 0, \
                    f"{env} seed {seed:#x}: {bad.size} blocks differ, " \
                    f"first {bad[:8]}"
