"""tests/cpp/online_endpoint_example.cc: the C++ mirror of endpointing (pocketkaldi::OnlineDecoder::SetEndpointing /
Endpoint / Finish, pocketkaldi::OnlineRecognizer::SetEndpointing / Utterances) compiles against the header and links
against the library; --link-only also tries the host-only rule test."""
import subprocess

from test_cpp_stream import build


def test_online_endpoint_example_compiles_and_links():
    assert "pk_mi355" in subprocess.check_output([build("online_endpoint_example"), "--link-only"], text=True)
