"""Compute ops: hand-written gfx950 HIP kernels (libgmt) behind torch-facing wrappers.

Kernel inventory: K1/K2 ``daxpy``; K3 ``stencil5_1d``;
K4/K5/K11 ``stencil5_2d`` (and its ``stencil5_2d_edges`` /
``stencil5_2d_interior`` split for overlapped steps); K6/K7/K8 ``copy2d_batched`` (halo pack/unpack);
K9 ``sum_axis``; K10/K12 ``diff_sq``/``diff_norm``; analytic ``fill_poly``;
and the BASELINE 5-point Jacobi ``jacobi5`` / ``jacobi5_rects`` (single sweep),
its read-only residual ``jacobi5_resid``, the conjugate-gradient launches
``cg_apply`` / ``cg_update`` / ``cg_dir``, the Chebyshev step ``cheby_step``,
the multigrid smoother and grid transfers ``mg_smooth`` / ``mg_restrict`` /
``mg_prolong_add``, the fused smoother ``mg_smooth_k`` (k sweeps per memory
pass), the red-black Gauss-Seidel smoother ``mg_smooth_rb`` (h coloured
half-sweeps per memory pass), the fused residual + restriction
``mg_resid_restrict``, the fused interpolation + smoothing pass
``mg_prolong_smooth``, the table-driven transfers for levels that are not nested
``mg_restrict_tab`` / ``mg_prolong_add_tab``, and ``jacobi5tb`` (K fused sweeps
per memory pass).
"""
from .kernels import (  # noqa: F401
    abs_max,
    add2d,
    add2d_path,
    cg_apply,
    cg_apply_path,
    cg_dir,
    cg_dir_path,
    cg_update,
    cg_update_path,
    cheby_step,
    cheby_step_path,
    copy2d_batched,
    daxpy,
    diff_norm,
    diff_bits,
    diff_sq,
    xcd_of_workgroups,
    fill_poly,
    PATH_D1_DMA,
    PATH_D1_WIN,
    PATH_NONE,
    PATH_PT,
    PATH_ROW_WALK,
    PATH_SCALAR,
    jacobi5,
    jacobi5_path,
    jacobi5_rects,
    jacobi5_resid,
    jacobi5_resid_path,
    mg_prolong_add,
    mg_prolong_add_path,
    mg_prolong_add_tab,
    mg_prolong_add_tab_path,
    mg_prolong_smooth,
    mg_prolong_smooth_geom,
    mg_prolong_smooth_path,
    mg_resid_restrict,
    mg_resid_restrict_geom,
    mg_resid_restrict_path,
    mg_restrict,
    mg_restrict_path,
    mg_restrict_tab,
    mg_restrict_tab_path,
    mg_smooth,
    mg_smooth_k,
    mg_smooth_k_geom,
    mg_smooth_k_path,
    mg_smooth_path,
    mg_smooth_rb,
    mg_smooth_rb_path,
    jacobi5xk,
    jacobi5tb,
    jacobi5tb_plan,
    jacobi5tb_shared_geom,
    jacobi5tb_shared_path,
    tb_push_shared_supported,
    tb_supported,
    stencil5_1d,
    stencil5_2d,
    stencil5_2d_edges,
    stencil5_2d_interior,
    stencil5_2d_path,
    stencil5_bands,
    sum_axis,
    vsum,
)
from .reference import DERIV5  # noqa: F401
