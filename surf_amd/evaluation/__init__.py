"""Offline evaluation: DTU Chamfer distance, mask / visibility based mesh cleaning, and the Tanks and Temples F-score."""
