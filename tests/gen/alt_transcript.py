"""A second Fiat-Shamir transcript for the tests of plk_transcript_ops, in two faces over one core:

  AltOracle   what oracle/plonk_oracle.py constructs as `Transcript()` once a test has substituted it (monkeypatch.setattr(po,
              "Transcript", AltOracle)): absorb_fr(int), absorb_g1(point), challenge() -> int;
  AltOps      a plonkit_amd.TranscriptOps for Context.set_transcript / verify(..., transcript=): the same hash fed from the bytes the
              library hands to its callbacks.

It differs from the rolling Keccak in every property a shortcut in the library could lean on: ONE 64-byte state instead of two 32-byte
ones, BLAKE2b, LITTLE-endian canonical bytes, a challenge that also UPDATES the state (no counter), and a challenge that is the
512-bit digest REDUCED mod r instead of masked to 253 bits — values >= 2^253 occur (about two in five).  The library's Montgomery
words are converted with plain Python integers (x * R^-1 mod r, mod q), not with the library.

Both faces append to `trace` (a list the test supplies): ("begin",), ("fr", v), ("g1", x, y), ("ch", c), canonical integers, and for
AltOps ("end",).  The Keccak faces at the bottom route the library's own rolling Keccak through the same callbacks."""
import hashlib

import numpy as np

from oracle import oracle_lib as ol
from oracle.oracle_lib import R_MOD, Q_MOD

R_INV = pow(1 << 256, -1, R_MOD)
RQ_INV = pow(1 << 256, -1, Q_MOD)


def fr_of_bytes(b):
    """32 bytes of the ABI's in-memory Fr (little-endian limbs, Montgomery) -> canonical integer"""
    return int.from_bytes(b, "little") * R_INV % R_MOD


def fr_to_abi(v):
    return ((v << 256) % R_MOD).to_bytes(32, "little")


def g1_of_bytes(b):
    """64 bytes x || y Montgomery Fq -> canonical (x, y); infinity is (0, 0)"""
    return int.from_bytes(b[:32], "little") * RQ_INV % Q_MOD, int.from_bytes(b[32:], "little") * RQ_INV % Q_MOD


class AltCore:
    def __init__(self, tag=b"alt transcript for tests"):
        self.state = hashlib.blake2b(tag, digest_size=64).digest()

    def fr(self, v):
        self.state = hashlib.blake2b(b"F" + self.state + v.to_bytes(32, "little"), digest_size=64).digest()

    def g1(self, x, y):
        self.state = hashlib.blake2b(b"G" + self.state + x.to_bytes(32, "little") + y.to_bytes(32, "little"), digest_size=64).digest()

    def challenge(self):
        d = hashlib.blake2b(b"C" + self.state, digest_size=64).digest()
        self.state = hashlib.blake2b(b"S" + self.state + d, digest_size=64).digest()
        return int.from_bytes(d, "little") % R_MOD


class AltOracle:
    """the oracle's face; `trace` is class-level because the oracle constructs the object itself"""
    trace = None

    def __init__(self):
        self.core = AltCore()
        if AltOracle.trace is not None:
            AltOracle.trace.append(("begin",))

    def absorb_fr(self, v):
        self.core.fr(v)
        if AltOracle.trace is not None:
            AltOracle.trace.append(("fr", v))

    def absorb_g1(self, p):
        x, y = (0, 0) if ol.g1_is_inf(p) else ol.g1_to_ints(p)
        self.core.g1(x, y)
        if AltOracle.trace is not None:
            AltOracle.trace.append(("g1", x, y))

    def challenge(self):
        c = self.core.challenge()
        if AltOracle.trace is not None:
            AltOracle.trace.append(("ch", c))
        return c


class _State:
    """what TranscriptOps.begin() returns: a core behind the byte interface, with an optional script.
    script: {k: value} replaces the k-th challenge (0-based) by a canonical integer, by raw 32 ABI bytes, or raises the exception
    given; fail_at: the 1-based position among the calls after begin (absorbs and challenges alike) that raises."""

    def __init__(self, core, trace, script, fail_at):
        self.core, self.trace, self.script, self.fail_at = core, trace, script or {}, fail_at
        self.calls = self.challenges = 0

    def _count(self):
        self.calls += 1
        if self.fail_at is not None and self.calls == self.fail_at:
            raise TranscriptBoom("scripted failure at call %d" % self.calls)

    def absorb_fr(self, b):
        self._count()
        v = fr_of_bytes(b)
        self.core.fr(v)
        self.trace.append(("fr", v))

    def absorb_g1(self, b):
        self._count()
        x, y = g1_of_bytes(b)
        self.core.g1(x, y)
        self.trace.append(("g1", x, y))

    def challenge(self):
        self._count()
        c = self.core.challenge()
        k, self.challenges = self.challenges, self.challenges + 1
        if k in self.script:
            s = self.script[k]
            if isinstance(s, BaseException):
                raise s
            if isinstance(s, bytes):
                self.trace.append(("ch", None))
                return s
            c = s
        self.trace.append(("ch", c))
        return fr_to_abi(c)

    def end(self):
        self.trace.append(("end",))


class TranscriptBoom(RuntimeError):
    pass


class AltOps:
    """TranscriptOps face of the alt transcript (duck-typed: the library asks for begin() only)"""

    def __init__(self, script=None, fail_at=None, fail_begin=False):
        self.trace, self.script, self.fail_at, self.fail_begin = [], script, fail_at, fail_begin

    def core(self):
        return AltCore()

    def begin(self):
        if self.fail_begin:
            raise TranscriptBoom("scripted failure in begin")
        self.trace.append(("begin",))
        return _State(self.core(), self.trace, self.script, self.fail_at)


class _KeccakCore:
    """the library's own rolling Keccak (plk_transcript_*) behind AltCore's interface"""

    def __init__(self):
        import plonkit_amd as pa
        self.t = pa.Transcript()

    def fr(self, v):
        self.t.absorb_fr(np.frombuffer(fr_to_abi(v), dtype=np.uint64))

    def g1(self, x, y):
        b = ((x << 256) % Q_MOD).to_bytes(32, "little") + ((y << 256) % Q_MOD).to_bytes(32, "little")
        self.t.absorb_g1(np.frombuffer(b, dtype=np.uint64))

    def challenge(self):
        return fr_of_bytes(self.t.challenge().tobytes())


class KeccakOps(AltOps):
    """Keccak routed through the callbacks: the callbacks call plk_transcript_*"""

    def core(self):
        return _KeccakCore()


PROVER_TRACE = ["begin", "fr"] + ["g1"] * 4 + ["ch", "ch", "g1", "ch"] + ["g1"] * 4 + ["ch"] + ["fr"] * 11 + ["ch"]
VERIFIER_TRACE = PROVER_TRACE + ["g1", "g1", "ch"]


def kinds(trace):
    return [t[0] for t in trace]
