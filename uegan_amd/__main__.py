"""`python -m uegan_amd --mode train|test ...` (uegan_amd/runner.py; flags: uegan_amd/config.py)"""
from .runner import main

if __name__ == "__main__":
    main()
