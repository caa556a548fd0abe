"""LoD2 building solids from the footprints, the roof planes of roofs_whu.py and the terrain: see ada_mvs_amd/lod2.py."""
import ada_mvs_amd  # noqa: F401  (registers the package directory `ada-mvs_amd`)
from ada_mvs_amd.lod2 import main

if __name__ == "__main__":
    main()
