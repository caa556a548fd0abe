"""Ground filter of dsm_whu.py's DSM into a bare-earth DTM and an nDSM: see ada_mvs_amd/dtm.py."""
import ada_mvs_amd  # noqa: F401  (registers the package directory `ada-mvs_amd`)
from ada_mvs_amd.dtm import main

if __name__ == "__main__":
    main()
