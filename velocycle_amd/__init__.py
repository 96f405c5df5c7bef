"""velocycle_amd: MI355X-native engine for VeloCycle's SVI hot path (phase / velocity inference).

The per-step ELBO + reparameterised gradient runs in hand-written HIP kernels for gfx950
(velocycle_amd/csrc -> libvelocycle_hip.so, C ABI in include/velocycle_hip.h); this package is the
Python host side mirroring the reference's `fit()` entry points.
"""
__version__ = "0.1.0"

# names served from their modules on first use (importing the package stays free of torch)
_LAZY = {"gene_harmonics_bootstrap": "gene_bootstrap", "GeneHarmonicBootstrap": "gene_bootstrap",
         "gene_harmonics_batched_bootstrap": "gene_bootstrap", "GeneBatchHarmonicBootstrap": "gene_bootstrap",
         "velocity_map_bootstrap": "kinetics_bootstrap", "VelocityMapBootstrap": "kinetics_bootstrap",
         "cell_angular_speed": "cell_speed", "grouped_angular_speed": "cell_speed", "CellSpeedFit": "cell_speed",
         "GroupSpeedFit": "cell_speed", "velocity_map_joint": "gene_joint", "GeneJointFit": "gene_joint",
         "JointVelocityMapFit": "gene_joint",            # (`gene_joint` itself is its module's name: velocycle_amd.gene_joint.gene_joint)
         "gene_joint_weighted": "joint_bootstrap", "gene_joint_bootstrap": "joint_bootstrap", "GeneJointBootstrap": "joint_bootstrap",
         "velocity_map_joint_bootstrap": "joint_bootstrap", "JointVelocityMapBootstrap": "joint_bootstrap"}
__all__ = sorted(_LAZY)


def __getattr__(name):
    if name in _LAZY:
        from importlib import import_module
        return getattr(import_module(f".{_LAZY[name]}", __name__), name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
