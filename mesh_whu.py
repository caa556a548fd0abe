"""TSDF meshing of fuse_whu.py's depth maps into a coloured triangle mesh: see ada_mvs_amd/mesh.py."""
import ada_mvs_amd  # noqa: F401  (registers the package directory `ada-mvs_amd`)
from ada_mvs_amd.mesh import main

if __name__ == "__main__":
    main()
