"""MI355X-native batched ideal-ballooning eigen-solver (hot path of rahulgaur104/ideal-ballooning-solver).

Importable as `ibs_amd` (see ibs_amd.py at the repository root; this directory's name is not a
valid Python identifier).
"""
from ._lib import IbsError, LIB_PATH, MEM_DEVICE, MEM_HOST, SYMBOLS  # noqa: F401
from .solver import Context, ScanPlan, default_context, VjpStatusWarning, CLUSTER_BIT, BASIS_BIT, OPEN_CLUSTER_BIT, MAX_MODES, MAX_STARTS  # noqa: F401
from .operators import gamma_ball_full, gamma_ball_full_many, marginal_dPdrho, local_eq_fold, local_eq_fold_tangent, local_eq_lam_grad, local_eq_ray_triples, local_eq_ray_nodes, dPdrho_of, uniform_spacing, make_obj_w_grad, theta_grid, NearestSigmaWarning  # noqa: F401
from .scan import BallooningScan, shard_surfaces, gather_surfaces, gather_rows_tensor, pick_start, pick_starts, row_peaks, polish_theta0, first_unstable, local_eq_first_up, polish_first_up, append_history, GEO_ORDER  # noqa: F401
from .geometry import SurfaceTables  # noqa: F401
from .config import ScanConfig, load_params_dict, theta_grid_for, create_history_placeholders, PARAMS_KEYS  # noqa: F401
from .lbfgsb import minimize2  # noqa: F401
from .objective import ballooning_objective, dof_fd_gradient, linearised_dof_gradient, linearised_margin_gradient, dof_steps, shard_dofs, allreduce_dof_vector, AdjointStep  # noqa: F401
