"""Mesh deformation (Kimera-PGMO's mesh update stage) on the device: vertices
are bound once to their robot's nearest keyframes in a time window and follow
every new trajectory by the weighted blend of the keyframes' rigid corrections
(kmx_mesh_* in include/kmx_abi.h, csrc/mesh.hip), and the deformation graph's
own optimisation over simplified mesh vertices with keyframe priors
(kmx_dgraph_*, csrc/dgraph.hip), whose nodes the deformer can bind to."""
from .deformer import MeshDeformer, corrections_from_atlas  # noqa: F401
from .graph import DeformationGraph, graph_from_mesh, simplify_voxel  # noqa: F401
