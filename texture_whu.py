"""Texturing of mesh_whu.py's mesh from predict's source images: see ada_mvs_amd/texture.py."""
import ada_mvs_amd  # noqa: F401  (registers the package directory `ada-mvs_amd`)
from ada_mvs_amd.texture import main

if __name__ == "__main__":
    main()
