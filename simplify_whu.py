"""Simplification of mesh_whu.py's mesh by quadric vertex clustering on a lattice: see ada_mvs_amd/simplify.py."""
import ada_mvs_amd  # noqa: F401  (registers the package directory `ada-mvs_amd`)
from ada_mvs_amd.simplify import main

if __name__ == "__main__":
    main()
