"""Mesh deformation (Kimera-PGMO's mesh update stage) on the device: vertices
are bound once to their robot's nearest keyframes in a time window and follow
every new trajectory by the weighted blend of the keyframes' rigid corrections
(kmx_mesh_* in include/kmx_abi.h, csrc/mesh.hip)."""
from .deformer import MeshDeformer, corrections_from_atlas  # noqa: F401
