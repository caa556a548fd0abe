"""Cleaning of mesh_whu.py's mesh, small components dropped and small holes closed: see ada_mvs_amd/clean.py."""
import ada_mvs_amd  # noqa: F401  (registers the package directory `ada-mvs_amd`)
from ada_mvs_amd.clean import main

if __name__ == "__main__":
    main()
