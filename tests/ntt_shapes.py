"""The NTT shapes that tests/test_gpu_parity.py compares bit for bit with the oracle, in one place:
tests/test_ntt_plan.py (CPU) checks that between them they reach every kernel the launch planner
(xfg-stark_amd/csrc/ntt_plan.hpp) can name, so a route of the dispatcher cannot go untested."""

# forward LDE, (n, blowup), three polynomials each: test_lde_kernel_matches_oracle
LDE_3POLY = [(8, 2), (64, 8), (256, 16), (1024, 4), (4096, 8), (1 << 15, 8), (1 << 16, 2), (1 << 17, 2), (1 << 19, 2),
             (1 << 20, 2), (1 << 21, 2),
             # forward ntt_pass_a<2> (n = 16, 32), <3> and <4> with the odd split, ntt_pass_b<6> and <7>
             (16, 2), (32, 8), (128, 2), (512, 8), (1 << 11, 2), (1 << 13, 8), (1 << 14, 2)]
# one polynomial: test_lde_kernel_tile_paths_match_oracle
LDE_1POLY = [(1 << 18, 2), (1 << 22, 2), (1 << 20, 16), (1 << 22, 4), (1 << 16, 4), (1 << 16, 16), (1 << 17, 8),
             (1 << 17, 16)]
# 2^16, (npoly, blowup): test_lde_launch_set_routes_match_oracle
LDE_2P16_SETS = [(32, 8), (32, 2), (32, 4), (33, 16), (28, 8)]
# 2^20, two polynomials, blowup: test_lde_r1024_kernels_two_polys_match_oracle
LDE_R1024_BLOWUPS = [8, 16]
# (n, npoly, blowup): the all-coset pass A followed by the generic pass B applying the four-step twiddles
# (tq_b) -- the production batch shapes at 2^17 and 2^18: test_lde_all_coset_generic_pass_b_matches_oracle
LDE_ALL_COSET_GENERIC_B = [(1 << 17, 16, 2), (1 << 17, 16, 4), (1 << 18, 8, 2), (1 << 18, 8, 4)]

# inverse, (n, off7), two polynomials: test_interpolate_kernel_matches_oracle
INTERPOLATE_2POLY = [(8, False), (64, True), (2048, False), (2048, True), (1 << 14, True), (1 << 17, True),
                     (1 << 19, True), (1 << 20, False), (1 << 21, True),
                     # the odd splits: inverse ntt_pass_a<2..7> with ntt_pass_b<3..8>
                     (32, True), (128, False), (512, True), (1 << 13, False), (1 << 15, True)]
# one polynomial: test_interpolate_kernel_tile_paths_match_oracle
INTERPOLATE_1POLY = [(1 << 18, True), (1 << 22, False)]


def launches():
    """(direction, log2 n, log2 blowup, polynomials) of every call above"""
    lg = lambda v: v.bit_length() - 1
    out = [("fwd", lg(n), lg(b), 3) for n, b in LDE_3POLY] + [("fwd", lg(n), lg(b), 1) for n, b in LDE_1POLY]
    out += [("fwd", 16, lg(b), k) for k, b in LDE_2P16_SETS] + [("fwd", 20, lg(b), 2) for b in LDE_R1024_BLOWUPS]
    out += [("fwd", lg(n), lg(b), k) for n, k, b in LDE_ALL_COSET_GENERIC_B]
    out += [("inv", lg(n), 0, 2) for n, _ in INTERPOLATE_2POLY] + [("inv", lg(n), 0, 1) for n, _ in INTERPOLATE_1POLY]
    return out
