"""The sun exposure of dsm_whu.py's DSM and roofs_whu.py's roof planes: horizon, sky-view factor, sun hours, direct and global energy:
see ada_mvs_amd/solar.py."""
import ada_mvs_amd  # noqa: F401  (registers the package directory `ada-mvs_amd`)
from ada_mvs_amd.solar import main

if __name__ == "__main__":
    main()
