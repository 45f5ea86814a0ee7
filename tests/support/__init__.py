"""What the test modules share.  A test module imports tests.helpers and tests.support.*, never another test module."""
