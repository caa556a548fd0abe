"""Accuracy, completeness and F-score of a cloud or mesh against a truth, on the GPU: see ada_mvs_amd/accuracy.py."""
import ada_mvs_amd  # noqa: F401  (registers the package directory `ada-mvs_amd`)
from ada_mvs_amd.accuracy import main

if __name__ == "__main__":
    main()
