"""Image orthophoto of predict's source images over dsm_whu.py's DSM: see ada_mvs_amd/ortho.py."""
import ada_mvs_amd  # noqa: F401  (registers the package directory `ada-mvs_amd`)
from ada_mvs_amd.ortho import main

if __name__ == "__main__":
    main()
