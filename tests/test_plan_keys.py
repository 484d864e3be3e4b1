"""The plan-cache keys of lizardfs_amd.ec (enc_plan_key, rec_plan_key,
mix_plan_key): a cached plan holds device pointer arrays computed from
addresses, row strides, masks and geometry, so two calls that differ in any
one of those numbers must not share a key, and equal calls must.  Pure
functions of ints and tuples; no GPU."""
import pytest

pytest.importorskip("torch")     # lizardfs_amd.ec imports it

from lizardfs_amd import ec  # noqa: E402

ENC = dict(data_addr=0x7F0000001000, parity_addr=0x7F0000002000, S=3,
           plen=4096)
REC = dict(present=0b011101, nonnull=0b011101, needed=0b100010,
           src_addrs=(0x1000, 0x2000, 0x3000, 0x4000),
           src_strides=(8192, 8192, 4096, 8192),
           out_addrs=(0x9000, 0xA000), S=3, plen=4096)
MIX = dict(digest=bytes(range(16)),
           bases=(0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000),
           strides=(4096, 4096, 8192, 4096, 4096, 4096), out_addr=0x9000,
           S=3, plen=4096)
KINDS = {"enc": (ec.enc_plan_key, ENC), "rec": (ec.rec_plan_key, REC),
         "mix": (ec.mix_plan_key, MIX)}


def variants(args):
    """(what changed, args with exactly that one field changed): every
    scalar, and every element of every tuple, one at a time."""
    for name, v in args.items():
        if isinstance(v, tuple):
            for i in range(len(v)):
                w = list(v)
                w[i] += 16
                yield f"{name}[{i}]", dict(args, **{name: tuple(w)})
        elif isinstance(v, bytes):
            yield name, dict(args, **{name: bytes([v[0] ^ 1]) + v[1:]})
        elif name in ("present", "nonnull", "needed"):
            yield name, dict(args, **{name: v ^ 1})
        else:
            yield name, dict(args, **{name: v + 16})


@pytest.mark.parametrize("kind", tuple(KINDS))
def test_equal_inputs_equal_keys(kind):
    fn, args = KINDS[kind]
    a, b = fn(**args), fn(**{k: (list(v) if isinstance(v, tuple) else v)
                             for k, v in args.items()})
    assert a == b and hash(a) == hash(b)
    assert a[0] == kind


@pytest.mark.parametrize("kind", tuple(KINDS))
def test_one_changed_field_changes_the_key(kind):
    fn, args = KINDS[kind]
    base = fn(**args)
    seen = {base: "unchanged"}
    names = []
    for what, changed in variants(args):
        key = fn(**changed)
        assert key not in seen, f"{kind}: changing {what} gives the key of " \
                                f"{seen.get(key)}"
        seen[key] = what
        names.append(what.split("[")[0])
    # every field the issue lists was varied
    want = {"enc": {"data_addr", "parity_addr", "S", "plen"},
            "rec": {"present", "nonnull", "needed", "src_addrs",
                    "src_strides", "out_addrs", "S", "plen"},
            "mix": {"digest", "bases", "strides", "out_addr", "S",
                    "plen"}}[kind]
    assert set(names) == want


def test_kinds_do_not_collide():
    keys = {fn(**args) for fn, args in KINDS.values()}
    assert len(keys) == 3


def test_rec_key_tells_row_strides_apart():
    """Finding A: X[:, 0, :] of a [S, 2, L] tensor and X.view(2*S, L)[:S]
    share every address and differ only in row stride."""
    a = ec.rec_plan_key(**REC)
    b = ec.rec_plan_key(**dict(REC, src_strides=(4096,) * 4))
    assert a != b
