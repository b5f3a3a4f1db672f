"""Mesh deformation (Kimera-PGMO's mesh update stage) on the device: vertices
are bound once to their robot's nearest keyframes in a time window and follow
every new trajectory by the weighted blend of the keyframes' rigid corrections
(kmx_mesh_* in include/kmx_abi.h, csrc/mesh.hip), and the deformation graph's
own optimisation over simplified mesh vertices with keyframe priors
(kmx_dgraph_*, csrc/dgraph.hip), whose nodes the deformer can bind to. The
graph's control vertices and edges come from the mesh by voxel simplification:
in numpy on the host (simplify_voxel, graph_from_mesh: the reference) or on the
device, append by append (MeshSimplifier, simplify_voxel_gpu; kmx_simplify_*,
csrc/simplify.hip), with equal results."""
from .deformer import MeshDeformer, corrections_from_atlas  # noqa: F401
from .graph import DeformationGraph, graph_from_mesh, simplify_voxel  # noqa: F401
from .simplify import MeshSimplifier, simplify_voxel_gpu  # noqa: F401
