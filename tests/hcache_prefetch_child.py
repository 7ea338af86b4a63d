"""Child process of tests/test_gpu_hcache_prefetch.py: binds the library to two device contexts (both on device 0) and
checks that one hipbls_hcache_prefetch inserts the roots into EVERY context's H(m) cache: the host calls go round the
contexts, a queued hipbls_verify goes to the context its message hashes to, and all of them must hit.
"""
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

R_ORDER = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
OK, ERR_VERIFY = 0, 3


def main():
    from charon_amd.tbls import HipBLS
    impl = HipBLS(devices=[0, 0])
    assert impl.device_slots() == [0, 0]
    rng = random.Random(0x2C7)
    sks = [rng.randrange(1, R_ORDER).to_bytes(32, "big") for _ in range(2)]
    pks, st = impl.secret_to_public_key_batch(sks)
    assert set(st) == {OK}
    roots = [b"", rng.randbytes(32), rng.randbytes(200)]
    sigs, st = impl.sign_batch([sks[0]] * 3, roots)
    assert set(st) == {OK}
    assert impl.load_pubshares(list(pks)) == [OK, OK]
    try:
        impl.hcache_config(16)
        assert impl.hcache_prefetch(roots + roots[:1]) == (6, 0)  # three distinct roots, hashed in both contexts
        assert impl.hcache_stats() == (0, 0, 6)
        hits = 0
        for _ in range(2):  # two rounds of lone host calls: the round-robin reaches both contexts
            for r in range(3):
                assert impl.batch_verify_keys_status([0], [roots[r]], [sigs[r]]) == [OK]
                assert impl.batch_verify_keys_status([1], [roots[r]], [sigs[r]]) == [ERR_VERIFY]
                hits += 2
                assert impl.hcache_stats() == (hits, 0, 6)
        k0 = impl.queue_keyed_batches()
        for r in range(3):  # the queue: each root on the context it hashes to
            assert impl.verify_queued(pks[0], roots[r], sigs[r]) == OK
            hits += 1
            assert impl.hcache_stats() == (hits, 0, 6)
        assert impl.queue_keyed_batches() == k0 + 3
        assert impl.hcache_prefetch(roots) == (0, 6)
    finally:
        impl.hcache_config(0)
        impl.load_pubshares([])
    print("hcache prefetch child: 2 contexts ok")


if __name__ == "__main__":
    main()
