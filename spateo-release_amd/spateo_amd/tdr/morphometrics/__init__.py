from .model_morphology import model_morphology
from .morphofield import (
    _morphofield_sparsevfc,
    cell_directions,
    construct_genesis_states,
    morphofield_gp,
    morphofield_sparsevfc,
    morphopath,
)
from .morphofield_dg import (
    morphofield_acceleration,
    morphofield_curl,
    morphofield_curvature,
    morphofield_divergence,
    morphofield_jacobian,
    morphofield_torsion,
    morphofield_velocity,
)
from .morphology import cell_density, kernel_density, pc_KDE
from .shape_similarity import (
    calculate_eigenvector,
    model_eigenvector,
    pairwise_shape_similarity,
    shape_similarity_matrix,
    subspace_descriptors,
)
