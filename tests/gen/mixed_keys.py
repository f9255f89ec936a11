"""The keys of the mixed-batch tests (tests/test_gpu_verify_mixed.py, tests/test_verify_mixed_host.py), all forged by
tests/gen/forged_proofs.py from ONE set of random arguments so that each differs from key A in exactly one of the three things a lane
takes through its key index:

  A   n = 2^10 - 1, 2 inputs, tau = 42
  F   A with n = 2^11 - 1            only FrontVk differs (one byte of the vk); a proof of A is settled by the front end
  M   A with log(q_const) + 1        only one fixed point differs; the front end cannot see it, the proof reaches the pairing
  T   A with tau = 5                 only the G2 pair differs: a second line table

The proof forged for each is valid under its own key and invalid under each of the other three (checked on the oracle by cross_matrix)."""
import functools
import random

from oracle import plonk_oracle as po
from oracle.oracle_lib import R_MOD
from tests.gen import forged_proofs as fp

NAMES = ("A", "F", "M", "T")
TAU = {"A": 42, "F": 42, "M": 42, "T": 5}


def base_args():
    return fp.random_args(random.Random("the mixed batch"))


def args_of(name, base=None):
    a = dict(base if base is not None else base_args())
    if name == "F":
        a["n"] = (1 << 11) - 1
    elif name == "M":
        key = list(a["key_dlogs"])
        key[5] = (key[5] + 1) % R_MOD
        a["key_dlogs"] = key
    elif name == "T":
        a["tau"] = 5
    elif name != "A":
        raise KeyError(name)
    return a


@functools.lru_cache(maxsize=None)
def forged(name, variant=None):
    """-> Forged for key `name` with the shared data"""
    return fp.forge_record(**dict(args_of(name), variant=variant))


def more_proofs(name, count, seed):
    """`count` further valid proofs of key `name` (other proof data, the same key)"""
    rng = random.Random("more proofs %s %s" % (name, seed))
    own = args_of(name)
    out = []
    for _ in range(count):
        a = dict(fp.random_args(rng, key=own["key_dlogs"]), n=own["n"], tau=own.get("tau", 42))
        f = fp.forge_record(**a)
        assert f.vk == forged(name).vk and f.valid
        out.append(f.proof)
    return out


def cross_matrix():
    """verdict[p][k] of proof p under key k on the oracle: the identity"""
    return [[bool(po.verify(po.read_vk(forged(k).vk), po.read_proof(forged(p).proof), TAU[k])) for k in NAMES] for p in NAMES]
