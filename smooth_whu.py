"""Smoothing of mesh_whu.py's mesh by bilateral normal filtering: see ada_mvs_amd/smooth.py."""
import ada_mvs_amd  # noqa: F401  (registers the package directory `ada-mvs_amd`)
from ada_mvs_amd.smooth import main

if __name__ == "__main__":
    main()
