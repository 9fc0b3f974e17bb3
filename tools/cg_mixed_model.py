"""The bytes model tools/cg_mixed_bench.py holds its measurements against: what one iteration and one update of spmv_hip_cg_mixed move
through HBM, next to spmv_hip_cg's iteration on the fp64 handle.

A multiply's bytes are the schedule's own account (spmv_hip_info: stream_bytes + x_bytes).  The vector kernels of a CG iteration move 11
elements per row (tools/cg_bench.py: cg_dot reads p, q; cg_update reads p, q, x, r and writes x, r; cg_direction reads r, p and writes p), of
8 bytes in spmv_hip_cg on the fp64 handle and of 4 bytes in the mixed solve's iteration, which is the same three kernels on floats."""


def cg_iteration_bytes(spmv_bytes, m, elem):
    """one iteration of spmv_hip_cg: the multiply and 11 vector elements per row"""
    return spmv_bytes + 11 * elem * m


def mixed_iteration_bytes(low_spmv_bytes, m):
    """one iteration of spmv_hip_cg_mixed: fp32 CG's"""
    return cg_iteration_bytes(low_spmv_bytes, m, 4)


def update_bytes(high_spmv_bytes, m):
    """one update: the fp64 multiply and, per row, mix_try (x 8 + y 4 in, xn 8 out), mix_residual (b 8 + q64 8 in, r 4 out) and mix_resume
    (xn 8 in, x 8 + y 4 out): 60 bytes; a fresh direction (r 4 in, p 4 out) is the exception and not counted"""
    return high_spmv_bytes + 60 * m


def mixed_over_fp64(high_spmv_bytes, low_spmv_bytes, m, iterations_mixed, updates, iterations_fp64):
    """the model's time of a mixed solve over that of the fp64 solve, both as bytes"""
    mixed = iterations_mixed * mixed_iteration_bytes(low_spmv_bytes, m) + updates * update_bytes(high_spmv_bytes, m)
    return mixed / (iterations_fp64 * cg_iteration_bytes(high_spmv_bytes, m, 8))
