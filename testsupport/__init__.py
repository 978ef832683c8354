"""What the tests and the Python bench tools share, and neither owns: the geometry of a tree (treeshape), the numpy models that the
tests take their expected values from (forestappend, forestupdate, multiproofmodel) and one device helper (device).  Importable from the
repository root.  Nothing here imports from tests/ or bench_tools/; both import from here, and never from each other."""
