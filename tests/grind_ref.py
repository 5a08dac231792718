"""The proof-of-work search as winter-crypto states it, one hash at a time over the oracle's BLAKE3.

TEST INFRASTRUCTURE ONLY: the reference of tests/test_grinding_gpu.py and of the seed fixture
tests/golden/grind_seeds.json (tests/golden/make_grind_seeds.py). A call of oracle_lib.blake3 costs a few
microseconds from Python, so callers keep a test's searches under about a million hashes in all."""
import oracle_lib as O


def zeros(seed: bytes, nonce: int) -> int:
    """trailing zero bits of the first 8 LE bytes of BLAKE3(seed || nonce_le8); 64 for an all-zero word"""
    w = int.from_bytes(O.blake3(seed + nonce.to_bytes(8, "little"))[:8], "little")
    return 64 if w == 0 else (w & -w).bit_length() - 1


def min_nonce(seed: bytes, grind: int, first: int = 1, limit=None) -> int:
    """the smallest nonce in [first, limit] (limit None: unbounded) with zeros(seed, nonce) >= grind; 0 where
    the range holds none, as the device search reports it"""
    assert len(seed) == 32 and first >= 1
    nonce = first
    while limit is None or nonce <= limit:
        if zeros(seed, nonce) >= grind:
            return nonce
        nonce += 1
    return 0


def random_seeds(tag: str, count: int):
    """`count` reproducible 32-byte seeds"""
    return [O.blake3(f"grind-seed/{tag}/{i}".encode()) for i in range(count)]
