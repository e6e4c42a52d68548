"""Counterpart of cora.foreground: gaussianfg, galaxy (parameter classes), pointsource (unresolved background), poisson,
lofar (diffuse synchrotron from a spectral index per voxel)."""
