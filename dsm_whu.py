"""Rasterisation of fuse_whu.py's point cloud into a DSM and a true orthophoto: see ada_mvs_amd/dsm.py."""
import ada_mvs_amd  # noqa: F401  (registers the package directory `ada-mvs_amd`)
from ada_mvs_amd.dsm import main

if __name__ == "__main__":
    main()
